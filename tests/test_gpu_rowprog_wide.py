"""The conformer row programs (rowprog.hip) past FFN hidden 1024: the sizes TS-VAD's conformer back ends need
(transformer_ffn_embed_dim 1536).  The LDS parameter block holds two FFN slots of 3 * 384 + 1536 floats; the hidden layer
itself is produced 32 features at a time, so only the b1 slot and the piece count per tile grow with the hidden size.

Same op, references and error-model bounds as tests/test_gpu_rowprog.py (its run() and check(): max |Xo - emu64| <=
max |emu64 - ref64| and mean |Xo - emu64| <= mean |emu64 - ref64| / 10 per case; bf16 outputs atol 2e-2, rtol 1e-2).
Hidden 1056 is the first size past the old limit, 1536 the new one; M 40 is row-major with a dead tail, M 128 one whole
tile.  Hidden 1568 (a multiple of 32 past the limit) is refused with SD_ERR_INVALID before any launch."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_rowprog as rp  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

# (pre, n_ffn, y): one FFN (rowprog_ffn) | pre-GEMM + two FFNs + y (the middle layers' rowprog_pw2_ffn)
PROGRAMS = [(0, 1, 1), (1, 2, 1)]


@pytest.mark.parametrize("M", [40, 128])
@pytest.mark.parametrize("hidden", [1056, 1536])
@pytest.mark.parametrize("prog", PROGRAMS, ids=lambda p: "pre%d-ffn%d-y%d" % p)
def test_wide_hidden(gpu, prog, hidden, M):
    pre, n_ffn, y = prog
    X, p, ffns, yy = rp.make_program(31 * hidden + 7 * M + 100 * pre + n_ffn, M, pre, n_ffn, y, hidden)
    out = rp.run(gpu, M, X=X, pre=p, ffns=ffns, y=yy)
    rp.check(f"program {prog} hidden {hidden} M {M}", out, X.double(), p, ffns, yy)


@pytest.mark.parametrize("prog", PROGRAMS, ids=lambda p: "pre%d-ffn%d-y%d" % p)
def test_hidden_past_the_limit_is_refused(gpu, prog):
    """run() asserts that nothing was launched and no output row written."""
    pre, n_ffn, y = prog
    X, p, ffns, yy = rp.make_program(1568, 40, pre, n_ffn, y, 1568)
    assert rp.run(gpu, 40, X=X, pre=p, ffns=ffns, y=yy, expect=_lib.SD_ERR_INVALID) is None
