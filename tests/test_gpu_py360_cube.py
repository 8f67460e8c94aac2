"""pf_py360_e2c / pf_py360_c2e on the GPU: against the fixture of the reference's own external/py360convert within the
bounds of DESIGN.md 4.2 (tests/py360_cube_model.py ``check``), and against the float64 model in its tight form
(``check_tight``), which pins the addressing: pole rows, the seam, the appended rows and columns of every face."""
import ctypes as C

import numpy as np
import pytest
import torch

import py360_cube_model as M
from conftest import golden
from panfusion_amd import _lib
from panfusion_amd.external import py360convert as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORDER = {"bilinear": 1, "nearest": 0}
CASES = [(i, key, mode) for i in range(3) for key in ("u8", "f32") for mode in ("bilinear", "nearest")]


@pytest.fixture(scope="module")
def g():
    return golden("py360_cube.npz")


def _sub(setup, mask):
    P_, face, cy, cx = setup
    return P_, face[mask], cy[mask], cx[mask]


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("i,key,mode", CASES)
def test_e2c_vs_reference_fixture(g, i, key, mode):
    H, W, F = M.E2C_SHAPES[i]
    img, want = g["e2c_%d_%s_in" % (i, key)], g["e2c_%d_%s_%s" % (i, key, mode)]
    got = P.e2c(img, F, mode, "horizon")
    M.check(got, want, M.e2c_setup(img, F), ORDER[mode], float(g["e2c_%d_eps" % i]), "e2c %s %s %s" % ((H, W, F), key, mode))


@pytest.mark.parametrize("i,key,mode", CASES)
def test_c2e_vs_reference_fixture(g, i, key, mode):
    h, w, F = M.C2E_SHAPES[i]
    cube, want = g["c2e_%d_%s_in" % (i, key)], g["c2e_%d_%s_%s" % (i, key, mode)]
    got = P.c2e(cube, h, w, mode, "horizon")
    assert got.dtype == np.float64                                   # whatever the input dtype, like the reference
    M.check(got, want, M.c2e_setup(cube, h, w), ORDER[mode], float(g["c2e_%d_eps" % i]), "c2e %s %s %s" % ((h, w, F), key, mode))


# ------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("i,key,mode", CASES)
def test_e2c_kernel_vs_model(g, i, key, mode):
    F = M.E2C_SHAPES[i][2]
    img = g["e2c_%d_%s_in" % (i, key)]
    M.check_tight(P.e2c(img, F, mode, "horizon"), M.e2c_setup(img, F), ORDER[mode], "e2c %d %s %s" % (i, key, mode))


@pytest.mark.parametrize("out_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("i,key,mode", CASES)
def test_c2e_kernel_vs_model(g, i, key, mode, out_dtype):
    h, w, F = M.C2E_SHAPES[i]
    cube = g["c2e_%d_%s_in" % (i, key)]
    got = P.c2e(cube, h, w, mode, "horizon", out_dtype=out_dtype)
    assert got.dtype == out_dtype
    M.check_tight(got, M.c2e_setup(cube, h, w), ORDER[mode], "c2e %d %s %s" % (i, key, mode))


@pytest.mark.parametrize("Cc", [1, 3, 4])
def test_channel_counts_vs_model(Cc):
    rng = np.random.default_rng(40 + Cc)
    for mode, order in ORDER.items():
        img = (rng.random((33, 66, Cc)) * 255).astype(np.uint8)
        M.check_tight(P.e2c(img, 17, mode, "horizon"), M.e2c_setup(img, 17), order, "e2c C=%d %s" % (Cc, mode))
        cube = rng.standard_normal((13, 78, Cc)).astype(np.float32)
        M.check_tight(P.c2e(cube, 31, 56, mode, "horizon"), M.c2e_setup(cube, 31, 56), order, "c2e C=%d %s" % (Cc, mode))


# ------------------------------------------------------------------------------------------------ named hazards
@pytest.mark.parametrize("H,W,F", [(33, 66, 17), (47, 95, 31), (8, 16, 17)])
def test_e2c_up_and_down_faces_read_the_pole_rows(H, W, F):
    """Sampling rows above 0 / below H - 1 take rows H + 1 and H of the padded image: the first and last row rolled by
    W / 2.  An odd face has a pixel on the pole itself; the 8-row panorama has a disc of them."""
    img = np.random.default_rng(H).standard_normal((H, W, 2)).astype(np.float32)
    setup = M.e2c_setup(img, F)
    cy = setup[2]
    pole = (cy < 0) | (cy > H - 1)
    assert pole[:, 4 * F:5 * F].any() and pole[:, 5 * F:].any() and not pole[:, :4 * F].any()
    assert pole.sum() >= (18 if H == 8 else 2)
    got = P.e2c(img, F, "bilinear", "horizon")
    M.check_tight(got[pole], _sub(setup, pole), 1, "e2c poles %s" % ((H, W, F),), whole_image=False)
    # ... and the rolled rows matter: a model without the roll disagrees there
    flat = np.concatenate([img, img[[-1]], img[[0]]], 0).astype(np.float64)[None]
    assert np.abs(M.sample(flat, setup[1][pole], cy[pole], setup[3][pole], 1) - got[pole]).max() > 0.1


@pytest.mark.parametrize("i", range(3))
def test_e2c_back_face_straddles_the_seam(g, i):
    H, W, F = M.E2C_SHAPES[i]
    img = g["e2c_%d_u8_in" % i]
    setup = M.e2c_setup(img, F)
    seam = np.zeros(setup[3].shape, bool)
    seam[:, 2 * F:3 * F] = (setup[3][:, 2 * F:3 * F] < 1) | (setup[3][:, 2 * F:3 * F] > W - 2)
    assert seam.any()
    M.check_tight(P.e2c(img, F, "bilinear", "horizon")[seam], _sub(setup, seam), 1, "e2c seam %d" % i, whole_image=False)


@pytest.mark.parametrize("i", range(3))
def test_c2e_clipped_pixels_read_the_appended_rows_and_columns(g, i):
    """Coordinates clipped to 0 or face_w, and everything beyond face_w - 1, sample the rows and columns that
    sample_cubefaces appends from the neighbouring faces: on all six faces for the first two shapes, per-face distinct
    content."""
    h, w, F = M.C2E_SHAPES[i]
    cube = g["c2e_%d_f32_in" % i]
    setup = M.c2e_setup(cube, h, w)
    tp, cy, cx = setup[1:]
    pad = (cx > F - 1) | (cy > F - 1)
    clipped = (cx == 0) | (cx == F) | (cy == 0) | (cy == F)
    assert clipped.any() and all((pad & (tp == f)).any() for f in range(6 if i < 2 else 4))    # (31 x 56: U stays inside)
    got = P.c2e(cube, h, w, "bilinear", "horizon")
    M.check_tight(got[pad | clipped], _sub(setup, pad | clipped), 1, "c2e pads %d" % i, whole_image=False)
    # the appended samples come from OTHER faces: clamping to the face's own edge instead disagrees
    own = M.pad_cube(cube)
    own[:, F:, :], own[:, :, F:] = own[:, F - 1:F, :], own[:, :, F - 1:F]
    assert np.abs(M.sample(own, tp[pad], cy[pad], cx[pad], 1) - got[pad]).max() > 0.1


# ------------------------------------------------------------------------------------------------ the Python surface
def test_batched_calls_equal_single_calls(g):
    rng = np.random.default_rng(50)
    panos = (rng.random((3, 33, 66, 3)) * 255).astype(np.uint8)
    cubes = rng.standard_normal((3, 13, 78, 2)).astype(np.float32)
    for mode in ORDER:
        got = P.e2c_batch(panos, 17, mode)
        assert got.shape == (3, 17, 102, 3) and got.dtype == np.uint8
        for k in range(3):
            assert np.array_equal(got[k], P.e2c(panos[k], 17, mode, "horizon"))
        got = P.c2e_batch(cubes, 31, 56, mode)
        assert got.shape == (3, 31, 56, 2) and got.dtype == np.float64
        for k in range(3):
            assert np.array_equal(got[k], P.c2e(cubes[k], 31, 56, mode, "horizon"))
    assert not np.array_equal(got[0], got[1])


def test_tensor_in_tensor_out(g):
    img, cube = g["e2c_1_f32_in"], g["c2e_2_u8_in"]
    t = P.e2c(torch.from_numpy(img).to(DEV), 17, "bilinear", "horizon")
    assert t.is_cuda and t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), P.e2c(img, 17, "bilinear", "horizon"))
    dice = P.e2c(torch.from_numpy(img).to(DEV), 17)                   # default format, still on the device
    assert dice.is_cuda and np.array_equal(dice.cpu().numpy(), P.e2c(img, 17))
    for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32), (np.uint8, torch.uint8)):
        t = P.c2e(torch.from_numpy(cube).to(DEV), 31, 56, cube_format="horizon", out_dtype=dt)
        assert t.is_cuda and t.dtype == tdt
        assert np.array_equal(t.cpu().numpy(), P.c2e(cube, 31, 56, cube_format="horizon", out_dtype=dt))
    # a panorama becomes a skybox and comes back without leaving the device
    back = P.c2e(P.e2c(torch.from_numpy(img).to(DEV), 17), 33, 64, out_dtype=np.float32)
    assert back.is_cuda and tuple(back.shape) == (33, 64, 2)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("key", ["u8", "f32"])
def test_out_dtype_is_astype_of_the_float64_result(g, key, mode):
    for i, (h, w, F) in enumerate(M.C2E_SHAPES):
        cube = g["c2e_%d_%s_in" % (i, key)]
        if key == "f32":
            cube = np.abs(cube) * 30.0                               # (astype(uint8) is defined for values in [0, 256))
        full = P.c2e(cube, h, w, mode, "horizon")
        for dt in (np.float32, np.uint8):
            got = P.c2e(cube, h, w, mode, "horizon", out_dtype=dt)
            assert got.dtype == dt and np.array_equal(got, full.astype(dt)), (i, dt)
    assert (full != np.floor(full)).any() or mode == "nearest"       # uint8 truncated something


def test_cube_formats_equal_the_helpers_on_horizon(g):
    img, cube = g["e2c_1_u8_in"], g["c2e_1_u8_in"]
    hor = P.e2c(img, 17, "bilinear", "horizon")
    assert np.array_equal(P.e2c(img, 17), P.cube_h2dice(hor))       # 'dice' is the default
    lst, dct = P.e2c(img, 17, cube_format="list"), P.e2c(img, 17, cube_format="dict")
    assert len(lst) == 6 and all(np.array_equal(a, b) for a, b in zip(lst, P.cube_h2list(hor)))
    assert list(dct) == ["F", "R", "B", "L", "U", "D"] and all(np.array_equal(dct[k], v) for k, v in P.cube_h2dict(hor).items())
    want = P.c2e(cube, 16, 32, cube_format="horizon")
    for fmt in ("dice", "list", "dict"):
        assert np.array_equal(P.c2e(P.from_horizon(cube, fmt), 16, 32, cube_format=fmt), want), fmt
    assert np.array_equal(P.c2e(g["c2e_1_u8_in_dice"], 16, 32), want)
    from panfusion_amd.utils.pano import Cubemap, Equirectangular
    assert np.array_equal(Cubemap(cube, "horizon").to_equirectangular(16, 32).equirectangular, want)
    assert np.array_equal(Equirectangular(img).to_cubemap(17).cubemap, hor)


def test_c2e_more_workgroups_than_one_round_of_the_chip():
    """n = 2, face_w 128 -> 256 x 512: 1024 workgroups of 256 threads; the model on three row bands of both images."""
    rng = np.random.default_rng(60)
    level = np.repeat(np.array([20, 60, 100, 140, 180, 215]), 128)[None, None, :, None]
    cubes = (level + rng.random((2, 128, 768, 3)) * 40).astype(np.uint8)
    got = P.c2e_batch(cubes, 256, 512)
    assert got.shape == (2, 256, 512, 3) and got.dtype == np.float64
    for b in range(2):
        P_, tp, cy, cx = M.c2e_setup(cubes[b], 256, 512)
        for band in (slice(0, 6), slice(125, 131), slice(250, 256)):
            M.check_tight(got[b, band], (P_, tp[band], cy[band], cx[band]), 1, "c2e large image %d rows %s" % (b, band), whole_image=False)


def test_c_level_refusals_launch_nothing():
    lib = _lib.lib()
    rows = (C.c_int * 8)(*([4] * 8))
    msg = lambda: lib.pf_last_error_string()
    e2c_args = dict(img=0x10000, dtype=_lib.PF_U8, n=1, H=16, W=32, C=3, face_w=8, order=1, out=0x20000, stream=None)
    c2e_args = dict(cube=0x10000, dtype=_lib.PF_U8, n=1, face_w=8, C=3, rows=rows, h=16, w=32, order=1, out_dtype=_lib.PF_F64,
                    out=0x20000, stream=None)
    e2c = lambda **k: lib.pf_py360_e2c(*{**e2c_args, **k}.values())
    c2e = lambda **k: lib.pf_py360_c2e(*{**c2e_args, **k}.values())
    for kw, needle in ((dict(img=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(face_w=1), b"face_w"),
                       (dict(H=1), b"bad sizes"), (dict(W=1), b"bad sizes"), (dict(order=2), b"order"), (dict(dtype=_lib.PF_F16), b"dtype"),
                       (dict(dtype=_lib.PF_F64), b"dtype")):
        assert e2c(**kw) == 1 and b"pf_py360_e2c" in msg() and needle in msg(), (kw, msg())
    for kw, needle in ((dict(cube=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(rows=None), b"null pointer"),
                       (dict(face_w=1), b"face_w"), (dict(h=1), b"bad sizes"), (dict(w=36), b"multiple of 8"), (dict(order=3), b"order"),
                       (dict(dtype=_lib.PF_BF16), b"dtype"), (dict(out_dtype=_lib.PF_F16), b"out_dtype"),
                       (dict(rows=(C.c_int * 8)(*([17] * 8))), b"ceil_rows")):
        assert c2e(**kw) == 1 and b"pf_py360_c2e" in msg() and needle in msg(), (kw, msg())
    torch.cuda.synchronize()
