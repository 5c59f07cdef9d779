"""accflow_conv_wgrad_plan (csrc/backward.hip: conv_wgrad_plan, the host function accflow_conv_wgrad_f32 itself runs) on the
CPU: the refusals, the kernel choice at every edge of the fast kernel's predicate, the grid, and the pixel split - no part
shorter than 8 steps unless the whole problem is, the live parts cover every 16-pixel step exactly once.  The expected
values are stated for the default ACCFLOW_WGRAD_* knobs (the product build); tests/test_backward_routes.py pins its GPU
cases to these routes through the same query."""
import ctypes
import math

import pytest


@pytest.fixture(scope="module")
def lib():
    from accflow_amd import _lib
    return _lib.load()


GENERAL, FAST128, FAST64 = 0, 1, 2


def query(lib, B, Cin, Cout, H, W, KH, KW, s, pH, pW, x_bs=None, dy_bs=None, n=7):
    OH, OW = ((H + 2 * pH - KH) // s + 1, (W + 2 * pW - KW) // s + 1) if s > 0 else (0, 0)
    out = (ctypes.c_int * 8)(*([-7] * 8))
    rc = lib.accflow_conv_wgrad_plan(B, Cin, Cout, H, W, KH, KW, s, pH, pW, Cin * H * W if x_bs is None else x_bs,
                                     Cout * OH * OW if dy_bs is None else dy_bs, out, n)
    assert out[7] == -7                         # nothing past the seven documented fields
    return rc, list(out)[:7]


def plan(lib, *a, **k):
    rc, out = query(lib, *a, **k)
    assert rc == 0, (a, k)
    return dict(kernel=out[0], terms=out[1], gx=out[2], gy=out[3], Z=out[4], per=out[5], steps=out[6])


def cdiv(a, b):
    return -(-a // b)


def test_refusals(lib):
    ok = (2, 8, 40, 6, 16, 3, 3, 1, 1, 1)
    assert query(lib, *ok)[0] == 0
    for i in range(8):                          # B, Cin, Cout, H, W, KH, KW, stride: zero and negative
        for bad in (0, -1):
            a = list(ok)
            a[i] = bad
            rc, out = query(lib, *a)
            assert rc == 1 and out == [-7] * 7, (i, bad)
    assert query(lib, 2, 8, 40, 2, 16, 5, 3, 1, 0, 1)[0] == 1        # OH = 2 - 5 + 1 <= 0
    assert query(lib, 2, 8, 40, 6, 2, 3, 5, 1, 1, 0)[0] == 1         # OW <= 0
    assert query(lib, 2, 8, 40, 2, 16, 3, 3, 1, 0, 1)[0] == 1        # OH = 0 exactly
    assert query(lib, 2, 8, 40, 3, 16, 3, 3, 1, 0, 1)[0] == 0        # OH = 1
    rc, out = query(lib, *ok, n=6)                                   # too small an array: refused, untouched
    assert rc == 1 and out == [-7] * 7
    assert lib.accflow_conv_wgrad_plan(2, 8, 40, 6, 16, 3, 3, 1, 1, 1, 768, 3840, None, 7) == 1
    assert query(lib, *ok, n=8)[0] == 0


# B, Cin, Cout, H, W, KH, KW, stride, padH, padW -> kernel
KERNEL_EDGES = [
    ((2, 8, 40, 6, 16, 3, 3, 1, 1, 1), FAST64),
    ((2, 8, 40, 6, 8, 3, 3, 1, 1, 1), FAST64),
    ((2, 8, 40, 6, 12, 3, 3, 1, 1, 1), GENERAL),       # W % 8 = 4
    ((2, 8, 40, 6, 15, 3, 3, 1, 1, 1), GENERAL),       # W % 8 = 7
    ((2, 8, 40, 6, 17, 3, 3, 1, 1, 1), GENERAL),       # W % 8 = 1
    ((2, 8, 72, 6, 23, 3, 3, 1, 1, 1), GENERAL),
    ((2, 8, 40, 6, 16, 3, 3, 1, 1, 0), GENERAL),       # OW = W - 2
    ((2, 8, 40, 6, 10, 3, 3, 1, 1, 0), GENERAL),       # OW = 8: a multiple of 8, but not W
    ((2, 8, 40, 6, 16, 3, 3, 1, 0, 1), FAST64),        # only the width must be "same"
    ((2, 8, 40, 6, 16, 2, 3, 1, 0, 1), FAST64),
    ((2, 8, 40, 6, 16, 5, 5, 1, 2, 2), GENERAL),       # KW - 1 - padW = 2
    ((2, 8, 40, 6, 16, 1, 5, 1, 0, 2), GENERAL),
    ((2, 8, 40, 6, 16, 5, 1, 1, 2, 0), FAST64),        # a tall kernel is fine
    ((2, 8, 40, 6, 16, 1, 1, 1, 0, 0), FAST64),
    ((2, 8, 40, 6, 16, 1, 2, 1, 0, 0), GENERAL),       # KW = 2, padW = 0: OW = W - 1
    ((2, 8, 40, 6, 16, 3, 3, 2, 1, 1), GENERAL),       # stride 2 (OW = 8)
    ((2, 8, 40, 6, 16, 1, 1, 2, 0, 0), GENERAL),
    ((2, 8, 72, 6, 16, 3, 3, 2, 1, 1), GENERAL),
    ((2, 8, 1, 6, 16, 3, 3, 1, 1, 1), FAST64),
    ((2, 8, 64, 6, 16, 3, 3, 1, 1, 1), FAST64),        # Cout = 64: the last of the 64 x 256 tile
    ((2, 8, 65, 6, 16, 3, 3, 1, 1, 1), FAST128),       # Cout = 65
    ((2, 8, 128, 6, 16, 3, 3, 1, 1, 1), FAST128),
    ((2, 8, 129, 6, 16, 3, 3, 1, 1, 1), FAST128),
]


@pytest.mark.parametrize("case,kernel", KERNEL_EDGES)
def test_kernel_choice_and_grid(lib, case, kernel):
    B, Cin, Cout, H, W, KH, KW, s, pH, pW = case
    p = plan(lib, *case)
    assert p["kernel"] == kernel and p["terms"] == 3
    J = Cin * KH * KW
    assert (p["gx"], p["gy"]) == ((cdiv(J, 256), 1) if kernel == FAST64 else (cdiv(J, 128), cdiv(Cout, 128)))
    OH, OW = (H + 2 * pH - KH) // s + 1, (W + 2 * pW - KW) // s + 1
    assert p["steps"] == cdiv(B * OH * OW, 16)


@pytest.mark.parametrize("J,Cout,grid", [(128, 72, (1, 1)), (129, 72, (2, 1)), (256, 72, (2, 1)), (257, 72, (3, 1)),
                                         (128, 40, (1, 1)), (129, 40, (1, 1)), (256, 40, (1, 1)), (257, 40, (2, 1)),
                                         (257, 129, (3, 2)), (2313, 200, (19, 2))])
def test_tile_grid(lib, J, Cout, grid):
    p = plan(lib, 2, J, Cout, 6, 16, 1, 1, 1, 0, 0)
    assert (p["gx"], p["gy"]) == grid and p["kernel"] == (FAST64 if Cout <= 64 else FAST128)


def test_descriptor_limit_by_batch_stride(lib):
    """The fast kernel addresses both tensors through 32-bit buffer offsets: (B - 1) bs + C H W elements must stay below 2^31
    BYTES.  Reached by the batch stride of a (hypothetical) slice of a huge buffer - nothing is allocated."""
    case = (2, 8, 40, 6, 16, 3, 3, 1, 1, 1)
    x_last, dy_last = 2 ** 29 - 8 * 96 - 1, 2 ** 29 - 40 * 96 - 1      # the largest batch strides that still fit
    assert plan(lib, *case, x_bs=x_last)["kernel"] == FAST64
    assert plan(lib, *case, x_bs=x_last + 1)["kernel"] == GENERAL
    assert plan(lib, *case, dy_bs=dy_last)["kernel"] == FAST64
    assert plan(lib, *case, dy_bs=dy_last + 1)["kernel"] == GENERAL
    assert plan(lib, *case, x_bs=x_last, dy_bs=dy_last)["kernel"] == FAST64
    big = (2, 8, 72, 6, 16, 3, 3, 1, 1, 1)
    assert plan(lib, *big, x_bs=x_last)["kernel"] == FAST128 and plan(lib, *big, x_bs=2 ** 40)["kernel"] == GENERAL
    # with one item the stride does not count
    assert plan(lib, 1, 8, 40, 6, 16, 3, 3, 1, 1, 1, x_bs=2 ** 40, dy_bs=2 ** 40)["kernel"] == FAST64
    # the split does not depend on the route
    a, b = plan(lib, *case, x_bs=x_last), plan(lib, *case, x_bs=x_last + 1)
    assert (a["Z"], a["per"], a["steps"]) == (b["Z"], b["per"], b["steps"])


def expected_z(tiles, steps, target=512, catom=2.4):
    """The split with default knobs, restated: fill `target` workgroups (rounded down), at most sqrt(catom steps) parts, at
    least 8 steps per part."""
    z = 1 if tiles >= target else target // tiles
    z = min(z, max(1, int(math.sqrt(catom * steps))))
    if z * 8 > steps:
        z = max(1, steps // 8)
    return z


def parts(p):
    return [(z * p["per"], min((z + 1) * p["per"], p["steps"])) for z in range(p["Z"])]


# the pinned cases of tests/test_backward_routes.py: case -> kernel, steps, Z, steps per part, live parts
PINNED = [
    ((19, 8, 40, 7, 24, 3, 3, 1, 1, 1), FAST64, 200, 21, 10, 20),
    ((19, 8, 72, 7, 24, 3, 3, 1, 1, 1), FAST128, 200, 21, 10, 20),
    ((19, 8, 72, 7, 23, 3, 3, 1, 1, 1), GENERAL, 192, 21, 10, 20),
    ((13, 8, 72, 9, 24, 3, 3, 1, 1, 1), FAST128, 176, 20, 9, 20),
    ((11, 8, 72, 9, 23, 3, 3, 2, 1, 1), GENERAL, 42, 5, 9, 5),
    ((1, 8, 40, 1, 8, 3, 3, 1, 1, 1), FAST64, 1, 1, 1, 1),
    ((1, 8, 40, 3, 3, 3, 3, 1, 1, 1), GENERAL, 1, 1, 1, 1),
    ((2, 8, 40, 6, 16, 5, 5, 1, 2, 2), GENERAL, 12, 1, 12, 1),
    ((2, 8, 40, 6, 16, 3, 3, 1, 1, 0), GENERAL, 11, 1, 11, 1),
    ((2, 8, 40, 6, 16, 3, 3, 2, 1, 1), GENERAL, 3, 1, 3, 1),
]


@pytest.mark.parametrize("case,kernel,steps,Z,per,live", PINNED)
def test_pinned_splits(lib, case, kernel, steps, Z, per, live):
    p = plan(lib, *case)
    assert (p["kernel"], p["steps"], p["Z"], p["per"]) == (kernel, steps, Z, per)
    assert sum(1 for a, b in parts(p) if a < b) == live


def test_split_covers_every_step_once(lib):
    """Over a sweep of shapes (tiny to 10^5 steps, one to hundreds of tiles): Z 8 <= max(steps, 8), Z follows the stated rule,
    steps per part is what the kernels derive from gridDim.z, and the parts [z per, min((z + 1) per, steps)) that are not
    empty tile [0, steps) in order - no step twice, none missing; empty parts only at the end."""
    seen_empty = seen_many = 0
    for B in (1, 2, 3, 7, 19, 30):
        for (H, W) in ((1, 8), (3, 3), (7, 24), (9, 23), (32, 32), (64, 64), (96, 128), (17, 241)):
            for (Cin, Cout, K) in ((8, 40, 3), (8, 72, 3), (128, 256, 3), (1152, 128, 1), (257, 256, 3), (2, 128, 7)):
                for s in (1, 2):
                    pd = K // 2
                    if (H + 2 * pd - K) // s + 1 <= 0:
                        continue
                    p = plan(lib, B, Cin, Cout, H, W, K, K, s, pd, pd)
                    steps, Z, per = p["steps"], p["Z"], p["per"]
                    assert 1 <= Z and Z * 8 <= max(steps, 8), (B, H, W, Cin, Cout, K, s, p)
                    assert Z == expected_z(p["gx"] * p["gy"], steps), (B, H, W, Cin, Cout, K, s, p)
                    assert per == cdiv(steps, Z)
                    live = [(a, b) for a, b in parts(p) if a < b]
                    assert parts(p)[:len(live)] == live             # the empty parts trail
                    assert live[0][0] == 0 and live[-1][1] == steps
                    assert all(live[i][1] == live[i + 1][0] for i in range(len(live) - 1))
                    seen_empty += len(live) < Z
                    seen_many += Z > 100
    assert seen_empty > 0 and seen_many > 0     # the sweep reaches empty trailing parts and three-digit splits


def test_python_wrapper_matches_the_entry(lib):
    from accflow_amd import backward
    p = backward.conv_wgrad_plan(19, 8, 40, 7, 24, 3, 3, padding=1)
    assert p == {"kernel": "fast64", "terms": 3, "grid": (1, 1, 21), "steps_per_part": 10, "steps": 200}
    assert backward.conv_wgrad_plan(19, 8, 72, 7, 23, 3, 3, padding=(1, 1))["kernel"] == "general"
    assert backward.conv_wgrad_plan(2, 8, 72, 6, 16, 3, 3, padding=1, x_bs=2 ** 29)["kernel"] == "general"
    assert backward.conv_wgrad_plan(11, 8, 72, 9, 23, 3, 3, stride=2, padding=1)["grid"] == (1, 1, 5)
    with pytest.raises(RuntimeError):
        backward.conv_wgrad_plan(2, 8, 40, 2, 16, 5, 3, padding=(0, 1))
    with pytest.raises(RuntimeError):
        backward.conv_wgrad_plan(2, 8, 40, 6, 16, 3, 3, stride=0)
