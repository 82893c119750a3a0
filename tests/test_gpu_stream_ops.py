"""The FS-EEND chunk-streaming kernels (csrc/stream_ops.hip) one by one, through their sd_op_* entry points, against the
float64 restatements of tests/stream_ops_ref.py (whose inputs test_stream_ops_host.py shows to be sharp enough: every
wrong implementation of its list is at least 10 bounds away).

Bounds (never taken from the GPU's output):
  fp32  max(1e-5 max(1, max |ref|), 8 x the largest error of the same formula run by torch in float32 on the same
        inputs), the second term computed here on the CPU; 8 covers __expf and the different summation order.
  bf16  the same, plus 2^-8 |ref element| per element for the one output rounding (half a bf16 ulp is at most 2^-8 of
        the value).  The reference's operands are rounded where the kernel reads bf16 (q / k / v or `t`, the weights);
        its output is NOT rounded as well: the 2^-8 term is that rounding, and against a rounded reference a value
        next to a rounding midpoint lands a whole ulp away (up to 2^-7 |ref|: 1.55 bounds at attn k255 on one MI355X
        run, a correct kernel).  ln_out is fp32 in every mode.
Every case prints torch-float32's and the GPU's largest error; MEASURED holds one MI355X run.

Instantiations and paths, and a case that reaches each:
  attn_decode_kernel<*, 1, false>          attn k256 / one_key / two_tiles_one_query, separate merge
  attn_decode_kernel<*, 8, false>          attn k63 (nq 2), k64_delay (nq 8)
  attn_decode_kernel<*, 32, false>         attn k65_slots (nq 9), k255 (nq 32)
  attn_decode_kernel<*, Q, true>           the same cases with `cnt`
  attn_decode_kernel<*, 1, true, true>     one_key (nh 4), k256 (nh 3), two_tiles_one_query (nh 1): min(hh, nh - 1)
  attn_combine_kernel<*>                   every attn case (no `cnt`)
  the wave loop's second tile              two_tiles_per_wave, two_tiles_one_query (8300 keys, 32 blocks)
  blocks that own no tile                  hollow_blocks (8 blocks, 70 keys), one_key
  delay != 0                               k64_delay, k257_delay
  slot_block_kernel<*, 2>                  slot (1, 1), (1, 2)
  slot_block_kernel<*, 4>                  slot (1, 3), (2, 2)
  slot_block_kernel<*, 6>                  slot (1, 5), (1, 6)
  slot_block_kernel<*, 8>                  slot (1, 7), (1, 8), (2, 4)
  slot_block_kernel<*, 16>                 slot (3, 3), (2, 6), (5, 3), (2, 8), (4, 4): the LayerNorm rows past 8 and
                                           the frame grouping with up to 5 frames
  ffn_pair_kernel<*, 1, 16, 128>           ffn n 1
  ffn_pair_kernel<*, 8, 32, 64>            ffn n 2, 3, 4, 7, 8 (merge rounds of 3 rows: 1, 1, 2, 3, 3 rounds)
  enc / dec finish, D 256 .. 1024          finisher cases
  kv_append / gather_window grid stride    the cases above 262144 units
(* = both element types.)
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_ops_ref as ref  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")

# one MI355X run: case -> (max |torch fp32 - float64|, max |GPU - float64|)
MEASURED = {
    'attn one_key fp32': (0.000e+00, 0.000e+00), 'attn one_key fp32 out-proj': (1.057e-06, 1.469e-06),
    'attn one_key bf16': (0.000e+00, 0.000e+00), 'attn one_key bf16 out-proj': (8.488e-07, 1.554e-02),
    'attn k63 fp32': (3.426e-06, 2.293e-06), 'attn k63 bf16': (1.772e-06, 1.105e-02),
    'attn k64_delay fp32': (3.695e-06, 3.148e-06), 'attn k64_delay bf16': (2.033e-06, 1.477e-02),
    'attn k65_slots fp32': (3.414e-06, 3.516e-06), 'attn k65_slots bf16': (2.575e-06, 1.489e-02),
    'attn k255 fp32': (6.848e-06, 6.502e-06), 'attn k255 bf16': (3.379e-06, 1.554e-02),
    'attn k256 fp32': (1.696e-06, 7.066e-07), 'attn k256 fp32 out-proj': (1.020e-06, 8.737e-07),
    'attn k256 bf16': (1.437e-06, 7.495e-03), 'attn k256 bf16 out-proj': (1.094e-06, 7.155e-03),
    'attn k257_delay fp32': (5.584e-06, 5.423e-06), 'attn k257_delay bf16': (3.217e-06, 1.265e-02),
    'attn hollow_blocks fp32': (6.688e-06, 7.165e-06), 'attn hollow_blocks bf16': (4.998e-06, 1.541e-02),
    'attn two_tiles_per_wave fp32': (6.435e-06, 6.286e-06), 'attn two_tiles_per_wave bf16': (1.461e-06, 5.620e-03),
    'attn two_tiles_one_query fp32': (3.770e-06, 1.283e-06),
    'attn two_tiles_one_query fp32 out-proj': (3.464e-06, 1.690e-06),
    'attn two_tiles_one_query bf16': (2.868e-06, 3.736e-03),
    'attn two_tiles_one_query bf16 out-proj': (2.587e-06, 3.641e-03), 'attn big_logit fp32': (7.070e-06, 6.832e-06),
    'attn big_logit bf16': (2.889e-06, 7.790e-03), 'slot (1, 1) t_none-w_fp32-o_fp32': (1.486e-06, 1.157e-06),
    'slot (1, 1) t_none-w_fp32-o_fp32 ln_out': (3.524e-07, 2.682e-07),
    'slot (1, 1) t_fp32-w_fp32-o_fp32': (1.475e-06, 1.475e-06),
    'slot (1, 1) t_fp32-w_fp32-o_fp32 ln_out': (2.189e-07, 4.259e-07),
    'slot (1, 1) t_bf16-w_bf16-o_bf16': (1.323e-06, 1.512e-02),
    'slot (1, 1) t_bf16-w_bf16-o_bf16 ln_out': (2.862e-07, 3.131e-07),
    'slot (1, 1) t_bf16-w_fp32-o_bf16': (1.297e-06, 1.286e-02),
    'slot (1, 1) t_bf16-w_fp32-o_bf16 ln_out': (2.862e-07, 3.131e-07),
    'slot (1, 1) t_fp32-w_bf16-o_fp32': (1.108e-06, 1.513e-06),
    'slot (1, 1) t_fp32-w_bf16-o_fp32 ln_out': (2.189e-07, 4.259e-07),
    'slot (1, 2) t_none-w_fp32-o_fp32': (2.377e-06, 2.985e-06),
    'slot (1, 2) t_none-w_fp32-o_fp32 ln_out': (3.761e-07, 2.038e-07),
    'slot (1, 2) t_fp32-w_fp32-o_fp32': (1.612e-06, 2.086e-06),
    'slot (1, 2) t_fp32-w_fp32-o_fp32 ln_out': (2.891e-07, 3.940e-07),
    'slot (1, 2) t_bf16-w_bf16-o_bf16': (2.412e-06, 1.552e-02),
    'slot (1, 2) t_bf16-w_bf16-o_bf16 ln_out': (2.591e-07, 3.013e-07),
    'slot (1, 2) t_bf16-w_fp32-o_bf16': (1.791e-06, 1.544e-02),
    'slot (1, 2) t_bf16-w_fp32-o_bf16 ln_out': (2.591e-07, 3.013e-07),
    'slot (1, 2) t_fp32-w_bf16-o_fp32': (1.607e-06, 1.960e-06),
    'slot (1, 2) t_fp32-w_bf16-o_fp32 ln_out': (2.891e-07, 3.940e-07),
    'slot (1, 3) t_none-w_fp32-o_fp32': (1.754e-06, 1.685e-06),
    'slot (1, 3) t_none-w_fp32-o_fp32 ln_out': (4.341e-07, 2.350e-07),
    'slot (1, 3) t_fp32-w_fp32-o_fp32': (1.737e-06, 1.597e-06),
    'slot (1, 3) t_fp32-w_fp32-o_fp32 ln_out': (3.817e-07, 3.942e-07),
    'slot (1, 3) t_bf16-w_bf16-o_bf16': (3.074e-06, 1.527e-02),
    'slot (1, 3) t_bf16-w_bf16-o_bf16 ln_out': (4.392e-07, 5.026e-07),
    'slot (1, 3) t_bf16-w_fp32-o_bf16': (3.595e-06, 1.363e-02),
    'slot (1, 3) t_bf16-w_fp32-o_bf16 ln_out': (4.392e-07, 5.026e-07),
    'slot (1, 3) t_fp32-w_bf16-o_fp32': (1.629e-06, 1.566e-06),
    'slot (1, 3) t_fp32-w_bf16-o_fp32 ln_out': (3.817e-07, 3.942e-07),
    'slot (2, 2) t_none-w_fp32-o_fp32': (3.938e-06, 2.224e-06),
    'slot (2, 2) t_none-w_fp32-o_fp32 ln_out': (4.914e-07, 2.293e-07),
    'slot (2, 2) t_fp32-w_fp32-o_fp32': (4.961e-06, 1.786e-06),
    'slot (2, 2) t_fp32-w_fp32-o_fp32 ln_out': (3.725e-07, 4.177e-07),
    'slot (2, 2) t_bf16-w_bf16-o_bf16': (2.737e-06, 1.558e-02),
    'slot (2, 2) t_bf16-w_bf16-o_bf16 ln_out': (3.675e-07, 4.367e-07),
    'slot (2, 2) t_bf16-w_fp32-o_bf16': (2.887e-06, 1.454e-02),
    'slot (2, 2) t_bf16-w_fp32-o_bf16 ln_out': (3.675e-07, 4.367e-07),
    'slot (2, 2) t_fp32-w_bf16-o_fp32': (3.366e-06, 1.851e-06),
    'slot (2, 2) t_fp32-w_bf16-o_fp32 ln_out': (3.725e-07, 4.177e-07),
    'slot (1, 5) t_none-w_fp32-o_fp32': (3.755e-06, 2.719e-06),
    'slot (1, 5) t_none-w_fp32-o_fp32 ln_out': (4.476e-07, 3.248e-07),
    'slot (1, 5) t_fp32-w_fp32-o_fp32': (2.885e-06, 2.614e-06),
    'slot (1, 5) t_fp32-w_fp32-o_fp32 ln_out': (4.185e-07, 4.185e-07),
    'slot (1, 5) t_bf16-w_bf16-o_bf16': (4.322e-06, 1.543e-02),
    'slot (1, 5) t_bf16-w_bf16-o_bf16 ln_out': (5.287e-07, 3.187e-07),
    'slot (1, 5) t_bf16-w_fp32-o_bf16': (3.384e-06, 1.534e-02),
    'slot (1, 5) t_bf16-w_fp32-o_bf16 ln_out': (5.287e-07, 3.187e-07),
    'slot (1, 5) t_fp32-w_bf16-o_fp32': (3.365e-06, 2.851e-06),
    'slot (1, 5) t_fp32-w_bf16-o_fp32 ln_out': (4.185e-07, 4.185e-07),
    'slot (1, 6) t_none-w_fp32-o_fp32': (4.297e-06, 4.049e-06),
    'slot (1, 6) t_none-w_fp32-o_fp32 ln_out': (4.052e-07, 2.845e-07),
    'slot (1, 6) t_fp32-w_fp32-o_fp32': (4.146e-06, 2.683e-06),
    'slot (1, 6) t_fp32-w_fp32-o_fp32 ln_out': (4.535e-07, 5.411e-07),
    'slot (1, 6) t_bf16-w_bf16-o_bf16': (4.604e-06, 1.526e-02),
    'slot (1, 6) t_bf16-w_bf16-o_bf16 ln_out': (5.125e-07, 4.492e-07),
    'slot (1, 6) t_bf16-w_fp32-o_bf16': (4.498e-06, 1.472e-02),
    'slot (1, 6) t_bf16-w_fp32-o_bf16 ln_out': (5.125e-07, 4.492e-07),
    'slot (1, 6) t_fp32-w_bf16-o_fp32': (3.096e-06, 3.009e-06),
    'slot (1, 6) t_fp32-w_bf16-o_fp32 ln_out': (4.535e-07, 5.411e-07),
    'slot (1, 7) t_none-w_fp32-o_fp32': (5.884e-06, 2.422e-06),
    'slot (1, 7) t_none-w_fp32-o_fp32 ln_out': (4.972e-07, 3.773e-07),
    'slot (1, 7) t_fp32-w_fp32-o_fp32': (2.894e-06, 3.085e-06),
    'slot (1, 7) t_fp32-w_fp32-o_fp32 ln_out': (3.705e-07, 3.947e-07),
    'slot (1, 7) t_bf16-w_bf16-o_bf16': (3.013e-06, 1.552e-02),
    'slot (1, 7) t_bf16-w_bf16-o_bf16 ln_out': (4.236e-07, 4.362e-07),
    'slot (1, 7) t_bf16-w_fp32-o_bf16': (2.901e-06, 1.557e-02),
    'slot (1, 7) t_bf16-w_fp32-o_bf16 ln_out': (4.236e-07, 4.362e-07),
    'slot (1, 7) t_fp32-w_bf16-o_fp32': (4.840e-06, 2.764e-06),
    'slot (1, 7) t_fp32-w_bf16-o_fp32 ln_out': (3.705e-07, 3.947e-07),
    'slot (1, 8) t_none-w_fp32-o_fp32': (4.013e-06, 4.235e-06),
    'slot (1, 8) t_none-w_fp32-o_fp32 ln_out': (6.258e-07, 3.489e-07),
    'slot (1, 8) t_fp32-w_fp32-o_fp32': (4.200e-06, 3.308e-06),
    'slot (1, 8) t_fp32-w_fp32-o_fp32 ln_out': (4.816e-07, 4.515e-07),
    'slot (1, 8) t_bf16-w_bf16-o_bf16': (3.915e-06, 1.501e-02),
    'slot (1, 8) t_bf16-w_bf16-o_bf16 ln_out': (5.461e-07, 4.449e-07),
    'slot (1, 8) t_bf16-w_fp32-o_bf16': (2.861e-06, 1.515e-02),
    'slot (1, 8) t_bf16-w_fp32-o_bf16 ln_out': (5.461e-07, 4.449e-07),
    'slot (1, 8) t_fp32-w_bf16-o_fp32': (5.348e-06, 2.715e-06),
    'slot (1, 8) t_fp32-w_bf16-o_fp32 ln_out': (4.816e-07, 4.515e-07),
    'slot (2, 4) t_none-w_fp32-o_fp32': (4.513e-06, 2.963e-06),
    'slot (2, 4) t_none-w_fp32-o_fp32 ln_out': (3.952e-07, 3.875e-07),
    'slot (2, 4) t_fp32-w_fp32-o_fp32': (4.391e-06, 2.886e-06),
    'slot (2, 4) t_fp32-w_fp32-o_fp32 ln_out': (5.208e-07, 4.813e-07),
    'slot (2, 4) t_bf16-w_bf16-o_bf16': (4.483e-06, 1.558e-02),
    'slot (2, 4) t_bf16-w_bf16-o_bf16 ln_out': (5.392e-07, 4.926e-07),
    'slot (2, 4) t_bf16-w_fp32-o_bf16': (3.753e-06, 1.553e-02),
    'slot (2, 4) t_bf16-w_fp32-o_bf16 ln_out': (5.392e-07, 4.926e-07),
    'slot (2, 4) t_fp32-w_bf16-o_fp32': (4.885e-06, 4.528e-06),
    'slot (2, 4) t_fp32-w_bf16-o_fp32 ln_out': (5.208e-07, 4.813e-07),
    'slot (3, 3) t_none-w_fp32-o_fp32': (4.934e-06, 4.457e-06),
    'slot (3, 3) t_none-w_fp32-o_fp32 ln_out': (3.738e-07, 4.446e-07),
    'slot (3, 3) t_fp32-w_fp32-o_fp32': (4.158e-06, 1.957e-06),
    'slot (3, 3) t_fp32-w_fp32-o_fp32 ln_out': (4.909e-07, 5.409e-07),
    'slot (3, 3) t_bf16-w_bf16-o_bf16': (3.168e-06, 1.552e-02),
    'slot (3, 3) t_bf16-w_bf16-o_bf16 ln_out': (3.516e-07, 6.574e-07),
    'slot (3, 3) t_bf16-w_fp32-o_bf16': (2.704e-06, 1.541e-02),
    'slot (3, 3) t_bf16-w_fp32-o_bf16 ln_out': (3.516e-07, 6.574e-07),
    'slot (3, 3) t_fp32-w_bf16-o_fp32': (3.687e-06, 1.982e-06),
    'slot (3, 3) t_fp32-w_bf16-o_fp32 ln_out': (4.909e-07, 5.409e-07),
    'slot (2, 6) t_none-w_fp32-o_fp32': (3.767e-06, 4.733e-06),
    'slot (2, 6) t_none-w_fp32-o_fp32 ln_out': (3.850e-07, 4.228e-07),
    'slot (2, 6) t_fp32-w_fp32-o_fp32': (4.903e-06, 3.473e-06),
    'slot (2, 6) t_fp32-w_fp32-o_fp32 ln_out': (4.707e-07, 4.697e-07),
    'slot (2, 6) t_bf16-w_bf16-o_bf16': (5.473e-06, 1.560e-02),
    'slot (2, 6) t_bf16-w_bf16-o_bf16 ln_out': (5.911e-07, 4.299e-07),
    'slot (2, 6) t_bf16-w_fp32-o_bf16': (4.291e-06, 1.553e-02),
    'slot (2, 6) t_bf16-w_fp32-o_bf16 ln_out': (5.911e-07, 4.299e-07),
    'slot (2, 6) t_fp32-w_bf16-o_fp32': (4.298e-06, 3.139e-06),
    'slot (2, 6) t_fp32-w_bf16-o_fp32 ln_out': (4.707e-07, 4.697e-07),
    'slot (5, 3) t_none-w_fp32-o_fp32': (3.045e-06, 3.900e-06),
    'slot (5, 3) t_none-w_fp32-o_fp32 ln_out': (4.225e-07, 4.515e-07),
    'slot (5, 3) t_fp32-w_fp32-o_fp32': (5.102e-06, 4.808e-06),
    'slot (5, 3) t_fp32-w_fp32-o_fp32 ln_out': (4.328e-07, 3.923e-07),
    'slot (5, 3) t_bf16-w_bf16-o_bf16': (4.526e-06, 1.545e-02),
    'slot (5, 3) t_bf16-w_bf16-o_bf16 ln_out': (4.377e-07, 4.022e-07),
    'slot (5, 3) t_bf16-w_fp32-o_bf16': (6.806e-06, 1.556e-02),
    'slot (5, 3) t_bf16-w_fp32-o_bf16 ln_out': (4.377e-07, 4.022e-07),
    'slot (5, 3) t_fp32-w_bf16-o_fp32': (3.882e-06, 5.131e-06),
    'slot (5, 3) t_fp32-w_bf16-o_fp32 ln_out': (4.328e-07, 3.923e-07),
    'slot (2, 8) t_none-w_fp32-o_fp32': (6.025e-06, 5.020e-06),
    'slot (2, 8) t_none-w_fp32-o_fp32 ln_out': (3.750e-07, 4.473e-07),
    'slot (2, 8) t_fp32-w_fp32-o_fp32': (4.471e-06, 4.452e-06),
    'slot (2, 8) t_fp32-w_fp32-o_fp32 ln_out': (3.970e-07, 4.655e-07),
    'slot (2, 8) t_bf16-w_bf16-o_bf16': (5.032e-06, 1.516e-02),
    'slot (2, 8) t_bf16-w_bf16-o_bf16 ln_out': (6.198e-07, 5.146e-07),
    'slot (2, 8) t_bf16-w_fp32-o_bf16': (7.315e-06, 1.537e-02),
    'slot (2, 8) t_bf16-w_fp32-o_bf16 ln_out': (6.198e-07, 5.146e-07),
    'slot (2, 8) t_fp32-w_bf16-o_fp32': (5.181e-06, 4.046e-06),
    'slot (2, 8) t_fp32-w_bf16-o_fp32 ln_out': (3.970e-07, 4.655e-07),
    'slot (4, 4) t_none-w_fp32-o_fp32': (5.075e-06, 3.353e-06),
    'slot (4, 4) t_none-w_fp32-o_fp32 ln_out': (5.310e-07, 3.147e-07),
    'slot (4, 4) t_fp32-w_fp32-o_fp32': (4.329e-06, 2.171e-06),
    'slot (4, 4) t_fp32-w_fp32-o_fp32 ln_out': (5.779e-07, 4.769e-07),
    'slot (4, 4) t_bf16-w_bf16-o_bf16': (5.117e-06, 1.559e-02),
    'slot (4, 4) t_bf16-w_bf16-o_bf16 ln_out': (4.256e-07, 4.167e-07),
    'slot (4, 4) t_bf16-w_fp32-o_bf16': (3.720e-06, 1.558e-02),
    'slot (4, 4) t_bf16-w_fp32-o_bf16 ln_out': (4.256e-07, 4.167e-07),
    'slot (4, 4) t_fp32-w_bf16-o_fp32': (4.424e-06, 4.007e-06),
    'slot (4, 4) t_fp32-w_bf16-o_fp32 ln_out': (5.779e-07, 4.769e-07),
    'ffn n 1 t_none-w_fp32-o_fp32': (6.797e-07, 3.346e-07),
    'ffn n 1 t_none-w_fp32-o_fp32 ln_out': (3.198e-07, 2.980e-07),
    'ffn n 1 t_fp32-w_fp32-o_fp32': (7.582e-07, 3.471e-07),
    'ffn n 1 t_fp32-w_fp32-o_fp32 ln_out': (3.345e-07, 1.775e-07),
    'ffn n 1 t_bf16-w_bf16-o_bf16': (7.442e-07, 3.827e-03),
    'ffn n 1 t_bf16-w_bf16-o_bf16 ln_out': (2.901e-07, 2.380e-07),
    'ffn n 1 t_bf16-w_fp32-o_bf16': (8.578e-07, 3.751e-03),
    'ffn n 1 t_bf16-w_fp32-o_bf16 ln_out': (2.901e-07, 2.380e-07),
    'ffn n 1 t_fp32-w_bf16-o_fp32': (5.203e-07, 2.836e-07),
    'ffn n 1 t_fp32-w_bf16-o_fp32 ln_out': (3.345e-07, 1.775e-07),
    'ffn n 2 t_none-w_fp32-o_fp32': (8.025e-07, 3.268e-07),
    'ffn n 2 t_none-w_fp32-o_fp32 ln_out': (2.780e-07, 3.149e-07),
    'ffn n 2 t_fp32-w_fp32-o_fp32': (8.169e-07, 4.420e-07),
    'ffn n 2 t_fp32-w_fp32-o_fp32 ln_out': (4.265e-07, 3.616e-07),
    'ffn n 2 t_bf16-w_bf16-o_bf16': (8.149e-07, 4.850e-03),
    'ffn n 2 t_bf16-w_bf16-o_bf16 ln_out': (3.936e-07, 4.718e-07),
    'ffn n 2 t_bf16-w_fp32-o_bf16': (8.910e-07, 3.827e-03),
    'ffn n 2 t_bf16-w_fp32-o_bf16 ln_out': (3.936e-07, 4.718e-07),
    'ffn n 2 t_fp32-w_bf16-o_fp32': (1.027e-06, 3.859e-07),
    'ffn n 2 t_fp32-w_bf16-o_fp32 ln_out': (4.265e-07, 3.616e-07),
    'ffn n 3 t_none-w_fp32-o_fp32': (7.036e-07, 3.039e-07),
    'ffn n 3 t_none-w_fp32-o_fp32 ln_out': (3.919e-07, 2.640e-07),
    'ffn n 3 t_fp32-w_fp32-o_fp32': (8.170e-07, 3.794e-07),
    'ffn n 3 t_fp32-w_fp32-o_fp32 ln_out': (3.864e-07, 5.217e-07),
    'ffn n 3 t_bf16-w_bf16-o_bf16': (8.026e-07, 7.186e-03),
    'ffn n 3 t_bf16-w_bf16-o_bf16 ln_out': (5.016e-07, 4.135e-07),
    'ffn n 3 t_bf16-w_fp32-o_bf16': (9.852e-07, 5.716e-03),
    'ffn n 3 t_bf16-w_fp32-o_bf16 ln_out': (5.016e-07, 4.135e-07),
    'ffn n 3 t_fp32-w_bf16-o_fp32': (9.099e-07, 3.861e-07),
    'ffn n 3 t_fp32-w_bf16-o_fp32 ln_out': (3.864e-07, 5.217e-07),
    'ffn n 4 t_none-w_fp32-o_fp32': (5.128e-07, 3.515e-07),
    'ffn n 4 t_none-w_fp32-o_fp32 ln_out': (4.802e-07, 3.814e-07),
    'ffn n 4 t_fp32-w_fp32-o_fp32': (5.700e-07, 4.164e-07),
    'ffn n 4 t_fp32-w_fp32-o_fp32 ln_out': (3.979e-07, 5.084e-07),
    'ffn n 4 t_bf16-w_bf16-o_bf16': (7.043e-07, 7.479e-03),
    'ffn n 4 t_bf16-w_bf16-o_bf16 ln_out': (2.810e-07, 4.181e-07),
    'ffn n 4 t_bf16-w_fp32-o_bf16': (5.551e-07, 5.146e-03),
    'ffn n 4 t_bf16-w_fp32-o_bf16 ln_out': (2.810e-07, 4.181e-07),
    'ffn n 4 t_fp32-w_bf16-o_fp32': (5.385e-07, 4.305e-07),
    'ffn n 4 t_fp32-w_bf16-o_fp32 ln_out': (3.979e-07, 5.084e-07),
    'ffn n 7 t_none-w_fp32-o_fp32': (1.188e-06, 4.019e-07),
    'ffn n 7 t_none-w_fp32-o_fp32 ln_out': (4.695e-07, 2.915e-07),
    'ffn n 7 t_fp32-w_fp32-o_fp32': (7.981e-07, 4.634e-07),
    'ffn n 7 t_fp32-w_fp32-o_fp32 ln_out': (4.507e-07, 4.936e-07),
    'ffn n 7 t_bf16-w_bf16-o_bf16': (8.791e-07, 3.901e-03),
    'ffn n 7 t_bf16-w_bf16-o_bf16 ln_out': (3.245e-07, 3.398e-07),
    'ffn n 7 t_bf16-w_fp32-o_bf16': (6.939e-07, 3.859e-03),
    'ffn n 7 t_bf16-w_fp32-o_bf16 ln_out': (3.245e-07, 3.398e-07),
    'ffn n 7 t_fp32-w_bf16-o_fp32': (9.401e-07, 3.429e-07),
    'ffn n 7 t_fp32-w_bf16-o_fp32 ln_out': (4.507e-07, 4.936e-07),
    'ffn n 8 t_none-w_fp32-o_fp32': (7.570e-07, 4.285e-07),
    'ffn n 8 t_none-w_fp32-o_fp32 ln_out': (5.957e-07, 4.024e-07),
    'ffn n 8 t_fp32-w_fp32-o_fp32': (6.165e-07, 4.560e-07),
    'ffn n 8 t_fp32-w_fp32-o_fp32 ln_out': (4.535e-07, 5.019e-07),
    'ffn n 8 t_bf16-w_bf16-o_bf16': (7.279e-07, 7.529e-03),
    'ffn n 8 t_bf16-w_bf16-o_bf16 ln_out': (4.185e-07, 4.343e-07),
    'ffn n 8 t_bf16-w_fp32-o_bf16': (5.627e-07, 7.699e-03),
    'ffn n 8 t_bf16-w_fp32-o_bf16 ln_out': (4.185e-07, 4.343e-07),
    'ffn n 8 t_fp32-w_bf16-o_fp32': (6.601e-07, 3.660e-07),
    'ffn n 8 t_fp32-w_bf16-o_fp32 ln_out': (4.535e-07, 5.019e-07), 'enc_finish D 256 c 1': (3.034e-07, 2.884e-07),
    'enc_finish D 256 c 3': (3.902e-07, 2.699e-07), 'enc_finish D 256 c 4': (4.017e-07, 4.017e-07),
    'enc_finish D 256 c 5': (3.643e-07, 3.130e-07), 'enc_finish D 256 c 32': (5.009e-07, 5.124e-07),
    'enc_finish D 512 c 1': (2.730e-07, 3.523e-07), 'enc_finish D 512 c 3': (4.038e-07, 3.540e-07),
    'enc_finish D 512 c 4': (3.340e-07, 3.743e-07), 'enc_finish D 512 c 5': (6.825e-07, 4.706e-07),
    'enc_finish D 512 c 32': (5.269e-07, 5.213e-07), 'enc_finish D 768 c 1': (4.139e-07, 4.653e-07),
    'enc_finish D 768 c 3': (4.055e-07, 4.604e-07), 'enc_finish D 768 c 4': (6.130e-07, 5.587e-07),
    'enc_finish D 768 c 5': (3.834e-07, 4.795e-07), 'enc_finish D 768 c 32': (5.734e-07, 7.439e-07),
    'enc_finish D 1024 c 1': (7.628e-07, 4.742e-07), 'enc_finish D 1024 c 3': (3.933e-07, 4.064e-07),
    'enc_finish D 1024 c 4': (3.733e-07, 3.073e-07), 'enc_finish D 1024 c 5': (5.101e-07, 4.395e-07),
    'enc_finish D 1024 c 32': (5.771e-07, 5.127e-07), 'dec_finish D 256 c 1 C 1': (3.272e-10, 3.272e-10),
    'dec_finish D 256 c 5 C 1': (1.243e-08, 9.549e-09), 'dec_finish D 256 c 1 C 6': (1.278e-08, 3.280e-09),
    'dec_finish D 256 c 3 C 6': (1.912e-08, 1.184e-08), 'dec_finish D 256 c 11 C 3': (2.890e-08, 1.180e-08),
    'dec_finish D 512 c 1 C 1': (2.261e-08, 2.577e-10), 'dec_finish D 512 c 5 C 1': (7.408e-09, 7.830e-09),
    'dec_finish D 512 c 1 C 6': (1.003e-08, 8.594e-09), 'dec_finish D 512 c 3 C 6': (1.572e-08, 7.736e-09),
    'dec_finish D 512 c 11 C 3': (1.239e-08, 1.012e-08), 'dec_finish D 768 c 1 C 1': (5.525e-09, 1.799e-09),
    'dec_finish D 768 c 5 C 1': (3.308e-09, 6.471e-09), 'dec_finish D 768 c 1 C 6': (6.831e-09, 6.463e-09),
    'dec_finish D 768 c 3 C 6': (7.682e-09, 1.467e-08), 'dec_finish D 768 c 11 C 3': (2.060e-08, 1.199e-08),
    'dec_finish D 1024 c 1 C 1': (1.261e-09, 2.465e-09), 'dec_finish D 1024 c 5 C 1': (3.609e-09, 7.546e-09),
    'dec_finish D 1024 c 1 C 6': (8.617e-09, 5.575e-09), 'dec_finish D 1024 c 3 C 6': (7.487e-09, 4.168e-09),
    'dec_finish D 1024 c 11 C 3': (7.332e-09, 1.111e-08),
}


def report(name, ref64, ref32, got, bf16):
    """Prints the case's errors and returns the worst |got - want| / bound."""
    want = ref64
    bound = ref.bound_of(ref64, ref32, bf16)
    e32 = float((ref32.double() - ref64).abs().max())
    got = got.double().cpu()
    e = float((got - want).abs().max())
    w = ref.worst(got, want, bound)
    print(f"MEASURED {name!r}: ({e32:.3e}, {e:.3e}),  # fp32 bound {float(bound.min()):.3e}, worst {w:.3f} bounds")
    return w


def put(t, gpu, bf16=False):
    return t.to(torch.bfloat16 if bf16 else torch.float32).contiguous().to(gpu)


def nans(gpu, *shape, bf16=False):
    return torch.full(shape, NAN, device=gpu, dtype=torch.bfloat16 if bf16 else torch.float32)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                              b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


# ---------------------------------------------------------------- attn_decode
_ATTN_REF = {}


def attn_ref(case, bf16):
    """(inputs, attention in float64 / float32, out-projection in float64 / float32), computed once per case."""
    key = (case.name, bf16)
    if key not in _ATTN_REF:
        q, k, v, wo, bo = case.inputs(bf16)
        a64 = ref.decode_attention(q, k, v, case.pos, case.scale, case.delay)
        a32 = ref.decode_attention(q, k, v, case.pos, case.scale, case.delay, torch.float32)
        _ATTN_REF[key] = ((q, k, v, wo, bo), a64, a32, ref.out_proj(a64, wo, bo), ref.out_proj(a32, wo, bo, torch.float32))
    return _ATTN_REF[key]


class AttnBuffers:
    """The case's operands laid out as the runner lays them out: q inside packed (q | k | v) rows of 3 D, K and V as the
    two halves of a 2 D-wide history row; "enc": sequences one after another, "dec": sequences = slots, a token's slots
    side by side (tokens nseq rows apart).  Two history rows past the last key hold NaN."""

    def __init__(self, case, q, k, v, gpu, bf16):
        nseq, nq, nh, total = case.nseq, case.nq, case.nh, case.total
        D = nh * ref.HD
        g = torch.Generator().manual_seed(5)
        qkv = torch.randn(nseq, nq, 3 * D, generator=g)
        qkv[:, :, :D] = q.reshape(nseq, nq, D)
        hist = torch.full((nseq, total + 2, 2 * D), NAN)
        hist[:, :total, :D] = k.reshape(nseq, total, D)
        hist[:, :total, D:] = v.reshape(nseq, total, D)
        self.dec = case.layout == "dec"
        if self.dec:
            qkv, hist = qkv.transpose(0, 1), hist.transpose(0, 1)
            self.q_tok, self.q_seq, self.kv_tok, self.kv_seq = nseq * 3 * D, 3 * D, nseq * 2 * D, 2 * D
            self.o_tok, self.o_seq = nseq * D, D
        else:
            self.q_tok, self.q_seq, self.kv_tok, self.kv_seq = 3 * D, nq * 3 * D, 2 * D, (total + 2) * 2 * D
            self.o_tok, self.o_seq = D, nq * D
        self.qkv, self.hist = put(qkv, gpu, bf16), put(hist, gpu, bf16)
        self.es = 2 if bf16 else 4
        self.case, self.gpu, self.bf16, self.D = case, gpu, bf16, D
        self.nb = _lib.load().sd_attn_decode_blocks(case.max_keys)
        self.ws_n = nseq * nh * self.nb * nq * (2 + ref.HD)
        self.pos = torch.tensor([case.pos], dtype=torch.int32, device=gpu)

    def new_out(self):
        n = self.case.nseq * self.case.nq * self.D
        return nans(self.gpu, n + 64, bf16=self.bf16)

    def logical(self, out):
        c = self.case
        o = out[:c.nseq * c.nq * self.D].float()
        o = o.view(c.nq, c.nseq, c.nh, ref.HD).transpose(0, 1) if self.dec else o.view(c.nseq, c.nq, c.nh, ref.HD)
        return o.cpu()

    def run(self, out, ws, cnt=None, proj=None):
        c = self.case
        flag = ctypes.c_int(-1)
        wo, bo, o2, ws2, cnt2 = proj if proj else (None,) * 5
        _lib.call("sd_op_attn_decode", self.qkv.data_ptr(), self.q_tok, self.q_seq, self.hist.data_ptr(),
                  self.hist.data_ptr() + self.D * self.es, self.kv_tok, self.kv_seq, out.data_ptr(), self.o_tok,
                  self.o_seq, c.nseq, c.nq, c.nh, c.scale, self.pos.data_ptr(), c.delay, c.max_keys, int(self.bf16),
                  ws.data_ptr(), self.nb, _lib.ptr(cnt), _lib.ptr(wo), _lib.ptr(bo), _lib.ptr(o2), _lib.ptr(ws2),
                  _lib.ptr(cnt2), ctypes.byref(flag), _lib.stream_ptr(self.gpu))
        torch.cuda.synchronize()
        return flag.value


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ref.ATTN_CASES, ids=lambda c: c.name)
def test_attn_decode(gpu, case, bf16):
    (q, k, v, wo, bo), a64, a32, p64, p32 = attn_ref(case, bf16)
    b = AttnBuffers(case, q, k, v, gpu, bf16)
    tag = f"attn {case.name} {'bf16' if bf16 else 'fp32'}"
    n_out = case.nseq * case.nq * b.D

    # separate combine launch
    ws = nans(gpu, b.ws_n + 64)
    out_sep = b.new_out()
    assert b.run(out_sep, ws) == 0
    assert all_nan(out_sep[n_out:]) and all_nan(ws[b.ws_n:])
    assert report(tag, a64, a32, b.logical(out_sep), bf16) <= 1.0

    # the last block merges: three launches on the same counters, never re-zeroed
    cnt = torch.zeros(case.nseq * case.nh, dtype=torch.int32, device=gpu)
    ws = nans(gpu, b.ws_n + 64)
    for _ in range(3):
        out = b.new_out()
        assert b.run(out, ws, cnt) == 0
        assert int(cnt.abs().sum()) == 0
        # combine_value runs on the same partials in both merges
        assert same_bits(out, out_sep), "fused and separate merge differ"
    assert all_nan(ws[b.ws_n:])

    # ... and the out-projection in the same launch (one query per sequence only)
    dwo, dbo = put(wo, gpu, bf16), put(bo, gpu)
    ws2 = nans(gpu, case.nseq * case.nh * case.nq * b.D + 64)
    cnt2 = torch.zeros(case.nseq, dtype=torch.int32, device=gpu)
    first = None
    for _ in range(3):
        out, o2 = b.new_out(), b.new_out()
        ran = b.run(out, ws, cnt, (dwo, dbo, o2, ws2, cnt2))
        assert ran == (1 if case.nq == 1 else 0)
        assert int(cnt.abs().sum()) == 0 and int(cnt2.abs().sum()) == 0
        if ran:
            assert all_nan(o2[n_out:])
            first = o2 if first is None else first
            assert same_bits(o2, first)
        else:
            assert same_bits(out, out_sep) and all_nan(o2)
    if case.nq == 1:
        got = first[:n_out].float().view(case.nseq, 1, b.D).cpu() if not b.dec else \
            first[:n_out].float().view(1, case.nseq, b.D).transpose(0, 1).cpu()
        assert report(tag + " out-proj", p64, p32, got, bf16) <= 1.0
    assert all_nan(ws2[case.nseq * case.nh * case.nq * b.D:])


# ---------------------------------------------------------------- fused blocks
def block_buffers(d, n, gpu, t_mode, w_bf16, out_bf16, wnames):
    D = 256
    dev = {k: put(d[k], gpu) for k in ("x", "g", "b")}
    dev["t"] = None if t_mode is None else put(d["t"], gpu, t_mode)
    for k in d:
        if k in wnames:
            dev[k] = put(d[k], gpu, w_bf16)
        elif k not in dev:
            dev[k] = put(d[k], gpu)
    dev["out"] = nans(gpu, n + 2, D, bf16=out_bf16)
    dev["ln_out"] = nans(gpu, n + 2, D)
    dev["cnt"] = torch.zeros(1, dtype=torch.int32, device=gpu)
    return dev


def slot_call(dev, ws, c, C, gpu, **over):
    p = dict(ln_x=dev["x"], ln_t=dev["t"], t_bf16=int(dev["t"] is not None and dev["t"].dtype == torch.bfloat16),
             g=dev["g"], b=dev["b"], eps=1e-5, ln_out=dev["ln_out"], w_in=dev["w_in"], b_in=dev["b_in"],
             w_out=dev["w_out"], b_out=dev["b_out"], w_bf16=int(dev["w_in"].dtype == torch.bfloat16), out=dev["out"],
             out_bf16=int(dev["out"].dtype == torch.bfloat16), ws=ws, cnt=dev["cnt"], c=c, C=C, D=256, nh=4, scale=0.125)
    p.update(over)
    ran = ctypes.c_int(-1)
    _lib.call("sd_op_stream_slot_block", *[v.data_ptr() if torch.is_tensor(v) else v for v in p.values()],
              ctypes.byref(ran), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return ran.value


def check_block(tag, dev, n, r64, r32, y64, y32, out_bf16, relaunch):
    """out and ln_out against the reference, the sentinel rows, the counter, and two more launches bit for bit."""
    assert int(dev["cnt"][0]) == 0
    out, y = dev["out"].clone(), dev["ln_out"].clone()
    assert all_nan(out[n:]) and all_nan(y[n:])
    w_out = report(tag, r64, r32, out[:n], out_bf16)
    w_y = report(tag + " ln_out", y64, y32, y[:n], False)
    for _ in range(2):
        dev["out"].fill_(NAN)
        dev["ln_out"].fill_(NAN)
        assert relaunch() == 1
        assert int(dev["cnt"][0]) == 0
        assert same_bits(dev["out"], out) and same_bits(dev["ln_out"], y)
    assert w_out <= 1.0 and w_y <= 1.0


def dtype_id(m):
    t, w, o = m
    return f"t_{'none' if t is None else 'bf16' if t else 'fp32'}-w_{'bf16' if w else 'fp32'}-o_{'bf16' if o else 'fp32'}"


@pytest.mark.parametrize("modes", ref.SLOT_DTYPES, ids=dtype_id)
@pytest.mark.parametrize("c,C", ref.SLOT_SHAPES)
def test_stream_slot_block(gpu, c, C, modes):
    t_mode, w_bf16, out_bf16 = modes
    n = c * C
    d = ref.block_inputs(n, 100 * c + C, t_mode, w_bf16, "slot")
    args = (d["x"], d["t"], d["g"], d["b"], d["w_in"], d["b_in"], d["w_out"], d["b_out"], c, C, 4, 0.125)
    r64, y64 = ref.slot_block(*args)
    r32, y32 = ref.slot_block(*args, dtype=torch.float32)
    dev = block_buffers(d, n, gpu, t_mode, w_bf16, out_bf16, ("w_in", "w_out"))
    ws = nans(gpu, 4 * n * 256 + 64)
    assert slot_call(dev, ws, c, C, gpu) == 1
    check_block(f"slot ({c}, {C}) {dtype_id(modes)}", dev, n, r64, r32, y64, y32, out_bf16,
                lambda: slot_call(dev, ws, c, C, gpu))
    assert all_nan(ws[4 * n * 256:])


def test_stream_slot_block_refusals(gpu):
    d = ref.block_inputs(16, 1, False, False, "slot")
    dev = block_buffers(d, 16, gpu, False, False, False, ("w_in", "w_out"))
    ws = nans(gpu, 4 * 16 * 256)
    shifted = lambda t: t.data_ptr() + 4      # noqa: E731  (4 bytes off a 16-byte boundary)
    for over in (dict(D=512, nh=8), dict(D=128, nh=2), dict(c=17, C=1), dict(c=1, C=9), dict(ws=None), dict(cnt=None),
                 dict(w_in=shifted(dev["w_in"])), dict(w_out=shifted(dev["w_out"])), dict(ln_x=shifted(dev["x"])),
                 dict(g=shifted(dev["g"])), dict(b=shifted(dev["b"])), dict(ln_out=shifted(dev["ln_out"]))):
        assert slot_call(dev, gpu=gpu, **dict(dict(ws=ws, c=2, C=6), **over)) == 0, over
        assert all_nan(dev["out"]) and all_nan(dev["ln_out"]) and all_nan(ws) and int(dev["cnt"][0]) == 0, over


def ffn_call(dev, ws, n, gpu, **over):
    p = dict(ln_x=dev["x"], ln_t=dev["t"], t_bf16=int(dev["t"] is not None and dev["t"].dtype == torch.bfloat16),
             g=dev["g"], b=dev["b"], eps=1e-5, ln_out=dev["ln_out"], w1=dev["w1"], b1=dev["b1"], w2=dev["w2"],
             b2=dev["b2"], w_bf16=int(dev["w1"].dtype == torch.bfloat16), out=dev["out"],
             out_bf16=int(dev["out"].dtype == torch.bfloat16), ws=ws, cnt=dev["cnt"], n=n, D=256, F=2048)
    p.update(over)
    ran = ctypes.c_int(-1)
    _lib.call("sd_op_stream_ffn_pair", *[v.data_ptr() if torch.is_tensor(v) else v for v in p.values()],
              ctypes.byref(ran), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return ran.value


@pytest.mark.parametrize("modes", ref.SLOT_DTYPES, ids=dtype_id)
@pytest.mark.parametrize("n", ref.FFN_ROWS)
def test_stream_ffn_pair(gpu, n, modes):
    t_mode, w_bf16, out_bf16 = modes
    d = ref.block_inputs(n, 300 + n, t_mode, w_bf16, "ffn")
    args = (d["x"], d["t"], d["g"], d["b"], d["w1"], d["b1"], d["w2"], d["b2"])
    r64, y64 = ref.ffn_pair(*args)
    r32, y32 = ref.ffn_pair(*args, dtype=torch.float32)
    hidden = torch.nn.functional.linear(y64, d["w1"].double(), d["b1"].double())
    assert bool((hidden[:, ::4] < 0).all()) and bool((hidden > 0).any())      # relu kills the biased units
    dev = block_buffers(d, n, gpu, t_mode, w_bf16, out_bf16, ("w1", "w2"))
    ws = nans(gpu, 128 * 8 * 256 + 64)
    assert ffn_call(dev, ws, n, gpu) == 1
    check_block(f"ffn n {n} {dtype_id(modes)}", dev, n, r64, r32, y64, y32, out_bf16, lambda: ffn_call(dev, ws, n, gpu))
    assert all_nan(ws[128 * 8 * 256:])


def test_stream_ffn_pair_refusals(gpu):
    d = ref.block_inputs(8, 2, False, False, "ffn")
    dev = block_buffers(d, 8, gpu, False, False, False, ("w1", "w2"))
    ws = nans(gpu, 128 * 8 * 256)
    for over in (dict(n=9), dict(F=1024), dict(w1=dev["w1"].data_ptr() + 4), dict(w2=dev["w2"].data_ptr() + 4)):
        assert ffn_call(dev, gpu=gpu, **dict(dict(ws=ws, n=8), **over)) == 0, over
        assert all_nan(dev["out"]) and all_nan(dev["ln_out"]) and all_nan(ws) and int(dev["cnt"][0]) == 0, over


# ---------------------------------------------------------------- finishers
def finish_inputs(rows, D, seed, t_mode):
    g = torch.Generator().manual_seed(seed)
    x, t = torch.randn(rows, D, generator=g) * 1.5, torch.randn(rows, D, generator=g)
    lg, lb = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    t = None if t_mode is None else ref.rb(t) if t_mode else t
    return x, t, lg, lb


T_MODES = [None, False, True]


@pytest.mark.parametrize("c", [1, 3, 4, 5, 32])
@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_stream_enc_finish(gpu, D, c):
    t_mode = T_MODES[(D // 256 + c) % 3]
    mirrored = (D // 256 + c) % 2 == 0
    x, t, lg, lb = finish_inputs(c, D, 500 + D + c, t_mode)
    y64, y32 = ref.ln_add(x, t, lg, lb, 1e-5, torch.float64), ref.ln_add(x, t, lg, lb, 1e-5, torch.float32)
    cur0 = 7
    hist = nans(gpu, cur0 + c + 3, D)
    state = torch.tensor([cur0, -5], dtype=torch.int32, device=gpu)
    dx, dg, db = put(x, gpu), put(lg, gpu), put(lb, gpu)
    dt = None if t is None else put(t, gpu, t_mode)
    _lib.call("sd_op_stream_enc_finish", dx.data_ptr(), _lib.ptr(dt), int(bool(t_mode)), dg.data_ptr(), db.data_ptr(),
              1e-5, c, D, hist.data_ptr(), state.data_ptr(), state.data_ptr() + 4 if mirrored else None,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert state.tolist() == [cur0 + c, cur0 + c if mirrored else -5]
    assert all_nan(hist[:cur0]) and all_nan(hist[cur0 + c:])
    assert report(f"enc_finish D {D} c {c}", y64, y32, hist[cur0:cur0 + c], False) <= 1.0


@pytest.mark.parametrize("c,C", [(1, 1), (5, 1), (1, 6), (3, 6), (11, 3)])
@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_stream_dec_finish(gpu, D, c, C):
    t_mode = T_MODES[(D // 256 + c * C) % 3]
    x, t, lg, lb = finish_inputs(c * C, D, 600 + D + c * C, t_mode)
    emb = torch.randn(c, D, generator=torch.Generator().manual_seed(D + c))
    emb = emb / emb.norm(dim=-1, keepdim=True)
    s64, s32 = ref.dec_scores(x, t, lg, lb, emb, C), ref.dec_scores(x, t, lg, lb, emb, C, dtype=torch.float32)
    scores = nans(gpu, c * C + 4)
    cur = torch.tensor([11], dtype=torch.int32, device=gpu)
    dx, dg, db, de = put(x, gpu), put(lg, gpu), put(lb, gpu), put(emb, gpu)
    dt = None if t is None else put(t, gpu, t_mode)
    _lib.call("sd_op_stream_dec_finish", dx.data_ptr(), _lib.ptr(dt), int(bool(t_mode)), dg.data_ptr(), db.data_ptr(),
              1e-5, c, C, D, de.data_ptr(), scores.data_ptr(), cur.data_ptr(), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert cur.tolist() == [11 + c] and all_nan(scores[c * C:])
    assert report(f"dec_finish D {D} c {c} C {C}", s64, s32, scores[:c * C], False) <= 1.0


# ---------------------------------------------------------------- copies (exact)
@pytest.mark.parametrize("rows,width,ld_src,mult,cursor", [
    (5, 2048, 3072, 1, 3),          # the K | V half of a (q | k | v) row of 3 x 256 floats
    (12, 1024, 1536, 6, 2),         # bf16 rows, 6 slots per frame: destination row 12
    (1030, 4096, 4416, 1, 1),       # 263680 16-byte units: more than the 1024 x 256 threads of the grid
])
def test_kv_append(gpu, rows, width, ld_src, mult, cursor):
    g = torch.Generator().manual_seed(rows)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, ld_src // 4), generator=g, dtype=torch.int32).to(gpu)
    ld_dst = width + 32
    r0 = cursor * mult
    dst = torch.full((r0 + rows + 3, ld_dst // 4), -7, dtype=torch.int32, device=gpu)
    cur = torch.tensor([cursor], dtype=torch.int32, device=gpu)
    off = 256      # the copied columns start inside the source row
    _lib.call("sd_op_kv_append", src.data_ptr() + off, ld_src, rows, width, dst.data_ptr(), ld_dst, cur.data_ptr(), mult,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    want = torch.full_like(dst, -7)
    want[r0:r0 + rows, :width // 4] = src[:, off // 4:(off + width) // 4]
    assert torch.equal(dst, want) and cur.tolist() == [cursor]


@pytest.mark.parametrize("name,cursor,n_valid,pad,rows,hist_rows", [
    ("before_start", 3, 40, 9, 23, 40),       # cursor - pad < 0
    ("past_valid", 30, 33, 9, 23, 40),        # the window runs past n_valid
    ("inside", 20, 40, 9, 19, 40),
    ("nothing_valid", 0, 0, 9, 19, 40),
    ("grid_stride", 5, 1000, 9, 1030, 1100),  # 1030 x 256 = 263680 elements
])
def test_gather_window(gpu, name, cursor, n_valid, pad, rows, hist_rows):
    D = 256
    hist = torch.randn(hist_rows, D, generator=torch.Generator().manual_seed(rows))
    want = ref.gather_window(hist, cursor, n_valid, pad, rows)
    dh = put(hist, gpu)
    dst = nans(gpu, rows + 1, D)
    state = torch.tensor([cursor, n_valid], dtype=torch.int32, device=gpu)
    _lib.call("sd_op_gather_window", dh.data_ptr(), D, state.data_ptr(), state.data_ptr() + 4, pad, rows, dst.data_ptr(),
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert torch.equal(dst[:rows].cpu(), want) and all_nan(dst[rows:]) and state.tolist() == [cursor, n_valid]


def test_cursor_advance(gpu):
    state = torch.tensor([5, -1, 9], dtype=torch.int32, device=gpu)
    st = _lib.stream_ptr(gpu)
    _lib.call("sd_op_cursor_advance", state.data_ptr(), 3, state.data_ptr() + 4, st)
    _lib.call("sd_op_cursor_advance", state.data_ptr() + 8, 32, None, st)
    _lib.call("sd_op_cursor_advance", state.data_ptr(), 1, None, st)
    torch.cuda.synchronize()
    assert state.tolist() == [9, 8, 41]
