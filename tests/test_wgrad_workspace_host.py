"""CPU: the workspace sizes of the weight gradients, chore_conv2d_wgrad_workspace_bytes and chore_gemm_tn_workspace_bytes (csrc/train_bwd.hip;
neither needs a handle or a device).  These byte counts are part of the C interface -- convblock.hip lays its own workspace out with
them, and every caller allocates by them -- so they are pinned here, shape by shape: the matrix of wgrad_cases.SHAPES, the 13 layer
shapes of scripts/wgrad_layer_ab.py at B = 4, and the products the heads' weight gradients were sent through chore_gemm_tn_f32 with
(dW_l = dZ_l^T H_(l-1) over the staged rows: 128 x 256, 128 x 96 and 128 x 128), beside the shapes of test_gemm_tn.

The expected numbers were generated ONCE from a build of commit 93fbcfb -- the last one whose workspace function and launcher each derived
kernel, tiling and share count on their own -- not from the code under test: a change of a number here is a change of the interface."""
import ast
import os
import re

import wgrad_cases as wc
from conftest import REPO

# (taps, B, H, W, Cin, Cout) -> bytes
CONV = {
    (9, 2, 20, 44, 64, 64): 5908480,        # r64_64
    (9, 1, 3, 5, 64, 64): 295424,           # t64_64
    (9, 2, 32, 64, 256, 128): 37765120,     # e256_128
    (9, 3, 30, 40, 256, 128): 37765120,     # u256_128
    (9, 3, 24, 96, 128, 64): 31878144,      # b128_64
    (9, 2, 24, 40, 64, 32): 443136,         # n64_32
    (9, 1, 5, 7, 32, 32): 36992,            # n32_32
    (9, 1, 130, 127, 128, 128): 37781504,   # p128_128
    (1, 2, 16, 32, 64, 128): 532480,        # o64_128
    (1, 2, 20, 44, 128, 256): 4227072,      # o128_256
    (1, 1, 8, 32, 128, 128): 528384,        # q128_128
    (1, 1, 7, 32, 128, 128): 264192,        # f128_128
    (1, 2, 12, 24, 128, 128): 1188864,      # l128_128
    (1, 2, 32, 64, 256, 256): 16842752,     # s256_256
    (1, 2, 10, 12, 32, 96): 25344,          # n32_96
    # scripts/wgrad_layer_ab.py: (taps, cin, cout, H) at B = 4
    (9, 4, 256, 256, 64, 64): 37814272,
    (9, 4, 128, 128, 128, 64): 37781504,
    (9, 4, 128, 128, 64, 64): 37814272,
    (9, 4, 128, 128, 128, 128): 37781504,
    (1, 4, 128, 128, 128, 256): 16908288,
    (9, 4, 128, 128, 256, 128): 37765120,
    (1, 4, 128, 128, 256, 256): 16842752,
    (9, 4, 64, 64, 256, 128): 37765120,
    (9, 4, 64, 64, 128, 64): 37781504,
    (9, 4, 64, 64, 64, 64): 37814272,
    (9, 4, 32, 32, 256, 128): 37765120,
    (9, 4, 32, 32, 128, 64): 18890752,
    (9, 4, 32, 32, 64, 64): 9453568,
}
LAYER_AB = [(9, 64, 64, 256), (9, 128, 64, 128), (9, 64, 64, 128), (9, 128, 128, 128), (1, 128, 256, 128), (9, 256, 128, 128), (1, 256, 256, 128),
            (9, 256, 128, 64), (9, 128, 64, 64), (9, 64, 64, 64), (9, 256, 128, 32), (9, 128, 64, 32), (9, 64, 64, 32)]
# (P, M, N) -> bytes
GEMM_TN = {
    (80000, 128, 256): 4194304,
    (80000, 128, 96): 4227072,
    (80000, 128, 128): 4194304,
    (20000, 128, 256): 4194304,
    (20000, 128, 96): 1916928,
    (20000, 128, 128): 2555904,
    (1, 32, 32): 4096,
    (1, 128, 96): 49152,
    (31, 32, 32): 4096,
    (31, 128, 96): 49152,
    (33, 32, 32): 4096,
    (33, 128, 96): 49152,
    (1000, 32, 32): 8192,
    (1000, 128, 96): 98304,
}


def _lib():
    from chore_amd import _lib
    return _lib.lib


def test_table_covers_the_matrix_and_the_layers():
    assert {(s["taps"], s["B"], s["H"], s["W"], s["cin"], s["cout"]) for s in wc.SHAPES} <= set(CONV)
    assert {(taps, 4, H, H, cin, cout) for taps, cin, cout, H in LAYER_AB} <= set(CONV)
    src = open(os.path.join(REPO, "scripts", "wgrad_layer_ab.py")).read()
    m = re.search(r"^LAYERS = (\[.*?\])$", src, re.S | re.M)
    assert m and ast.literal_eval(m.group(1)) == LAYER_AB      # the script's list, as it is written there
    assert len(CONV) == len(wc.SHAPES) + len(LAYER_AB)


def test_conv2d_wgrad_workspace_bytes():
    L = _lib()
    got = {k: L.chore_conv2d_wgrad_workspace_bytes(*k) for k in CONV}
    assert got == CONV, {k: (got[k], CONV[k]) for k in CONV if got[k] != CONV[k]}
    # refused: taps, channel counts no multiple of 32, an empty batch
    for k in ((4, 2, 16, 32, 64, 64), (9, 2, 16, 32, 48, 64), (1, 2, 16, 32, 64, 48), (9, 0, 16, 32, 64, 64), (9, -1, 16, 32, 64, 64)):
        assert L.chore_conv2d_wgrad_workspace_bytes(*k) == 0, k


def test_gemm_tn_workspace_bytes():
    L = _lib()
    got = {k: L.chore_gemm_tn_workspace_bytes(*k) for k in GEMM_TN}
    assert got == GEMM_TN, {k: (got[k], GEMM_TN[k]) for k in GEMM_TN if got[k] != GEMM_TN[k]}
    for k in ((16, 48, 32), (16, 32, 48), (0, 32, 32)):
        assert L.chore_gemm_tn_workspace_bytes(*k) == 0, k
