"""CPU-side guard for the fused FCM block kernel's band-top wait (fcm_conv.hip fcm_block_kernel): `s_waitcnt
vmcnt(HR2)` retires the next band's LDS-DMA loads only if every wave issues exactly HR2 vector-memory
instructions (the band's output stores) between those loads and the wait.  In the built gfx950 code object,
every path from the last DMA of an issue group to that wait must hold exactly HR2 buffer stores and no other
vector-memory instruction; a store that the compiler branched around, or a load it moved into the loop, fails."""
import glob
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_hazards  # noqa: E402

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(isa_hazards.LLVM, "llvm-objdump")),
                                reason="ROCm LLVM tools absent")
HR2 = {"ILi1E": 4, "ILi2E": 2}   # output rows per wave per band: FbGeom<SH>::R / 2
VMEM = ("buffer_", "global_", "scratch_", "flat_")


def _is_dma(mn, ops):
    return mn.startswith("buffer_load") and ops.rstrip().endswith("lds")


def _is_band_wait(ins, j, hr2):
    """The band-top sequence: s_waitcnt vmcnt(hr2); s_waitcnt lgkmcnt(0); s_barrier (the compiler's own waits
    for the weight loads are not followed by the barrier)."""
    want = [("s_waitcnt", f"vmcnt({hr2})"), ("s_waitcnt", "lgkmcnt(0)"), ("s_barrier", "")]
    return j + 2 < len(ins) and all(ins[j + k][0] == w[0] and ins[j + k][1].strip() == w[1] for k, w in enumerate(want))


def _paths_to_wait(ins, labels, start, hr2):
    """Vector-memory mnemonics on every path from ins[start] (a DMA) to the band-top wait; a path ends
    unreported at the next DMA (which starts its own walk) or at the end of the program."""
    out, stack, seen = [], [(start + 1, ())], set()
    while stack:
        j, vm = stack.pop()
        while j < len(ins):
            if (j, vm) in seen:
                break
            seen.add((j, vm))
            mn, ops = ins[j]
            if _is_dma(mn, ops) or mn == "s_endpgm":
                break
            if _is_band_wait(ins, j, hr2):
                out.append(vm)
                break
            if mn.startswith(VMEM):
                vm = vm + (mn,)
                if len(vm) > 4 * hr2:
                    out.append(vm)
                    break
            if mn == "s_branch":
                j = labels[ops.strip()]
                continue
            if mn.startswith("s_cbranch"):
                stack.append((labels[ops.strip()], vm))
            j += 1
    return out


@needs_llvm
def test_every_wave_issues_exactly_hr2_stores_between_dma_and_wait():
    objs = sorted(glob.glob(os.path.join(REPO, "speaker_diarization_amd", "lib", "obj", "fcm_conv.hip.*.o")))
    if not objs:
        pytest.skip("library not built")
    kernels = 0
    for name, ins, labels in isa_hazards.parse(isa_hazards.disassemble(objs[0])):
        m = re.search(r"fcm_block_kernel(ILi[12]E)", name)
        if not m:
            continue
        kernels += 1
        hr2 = HR2[m.group(1)]
        assert any(_is_band_wait(ins, j, hr2) for j in range(len(ins))), name
        walked = 0
        for i, (mn, ops) in enumerate(ins):
            if not _is_dma(mn, ops):
                continue
            for vm in _paths_to_wait(ins, labels, i, hr2):
                walked += 1
                assert len(vm) == hr2 and all(v.startswith("buffer_store") for v in vm), (name, i, vm)
        assert walked, name   # the loop's wait is reached from a DMA issue
    assert kernels == 2
