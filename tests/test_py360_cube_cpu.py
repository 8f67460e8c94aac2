"""Cube-map conversion without a GPU: the float64 model (tests/py360_cube_model.py) against the fixture the reference's own
external/py360convert wrote (tests/golden/py360_cube.npz, tools/make_golden_py360_cube.py) within the bounds and caps of
DESIGN.md 4.2; the cube-format helpers; Cubemap.from_mp3d_skybox; the refusals that need no kernel."""
import numpy as np
import pytest
import torch

import py360_cube_model as M
from conftest import golden
from panfusion_amd.external import py360convert as P

ORDER = {"bilinear": 1, "nearest": 0}
# nearest-mode share of excused pixels the reference run measured, per shape
E2C_TIES = (0.0833, 0.0392, 0.0109)
C2E_TIES = (0.0, 0.0, 0.1290)


@pytest.fixture(scope="module")
def g():
    return golden("py360_cube.npz")


def test_fixture_states_shapes_and_eps(g):
    assert [tuple(s) for s in g["e2c_shapes"]] == list(M.E2C_SHAPES) and [tuple(s) for s in g["c2e_shapes"]] == list(M.C2E_SHAPES)
    assert float(g["eps_factor"]) == M.EPS_FACTOR
    for path in ("e2c", "c2e"):
        for i in range(3):
            meas, eps = float(g["%s_%d_eps_meas" % (path, i)]), float(g["%s_%d_eps" % (path, i)])
            assert eps == M.EPS_FACTOR * meas
            assert 1e-7 < meas < 1e-5            # a few float32 ulps of a coordinate below 100: the premise of the bounds


@pytest.mark.parametrize("i", range(3))
def test_e2c_reference_coordinates_within_eps_meas_of_the_model(g, i):
    H, W, F = M.E2C_SHAPES[i]
    coor = g["e2c_%d_coor" % i]
    assert coor.dtype == np.float32 and coor.shape == (F, 6 * F, 2)
    cx, cy = M.e2c_coords(H, W, F)
    meas = max(np.abs(coor[..., 0] - cx).max(), np.abs(coor[..., 1] - cy).max())
    assert meas <= float(g["e2c_%d_eps_meas" % i]) * (1 + 1e-6)


@pytest.mark.parametrize("i", range(3))
def test_c2e_reference_coordinates_within_eps_meas_of_the_model(g, i):
    h, w, F = M.C2E_SHAPES[i]
    c32 = g["c2e_%d_coor" % i]
    assert c32.dtype == np.float32 and c32.shape == (h, w, 2)
    tp, cx, cy = M.c2e_coords(h, w, F)
    assert np.array_equal(tp, g["c2e_%d_tp" % i])
    rx, ry = (c32[..., 0].astype(np.float64) + 0.5) * F, (c32[..., 1].astype(np.float64) + 0.5) * F      # c2e.py:56-57
    assert max(np.abs(rx - cx).max(), np.abs(ry - cy).max()) <= float(g["c2e_%d_eps_meas" % i]) * (1 + 1e-6)
    # every face is used, and the clip to 0 / face_w (the pad rows and columns) is reached
    assert sorted(np.unique(tp)) == list(range(6))
    assert (cx == 0).any() or (cx == F).any() or (cy == 0).any() or (cy == F).any()


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("key", ["u8", "f32"])
@pytest.mark.parametrize("i", range(3))
def test_e2c_model_vs_reference_fixture(g, i, key, mode):
    H, W, F = M.E2C_SHAPES[i]
    img, want = g["e2c_%d_%s_in" % (i, key)], g["e2c_%d_%s_%s" % (i, key, mode)]
    assert img.shape[:2] == (H, W) and want.dtype == img.dtype
    share = M.check(M.e2c(img, F, ORDER[mode]), want, M.e2c_setup(img, F), ORDER[mode], float(g["e2c_%d_eps" % i]),
                    "e2c %d %s %s" % (i, key, mode))
    if mode == "nearest":
        assert abs(share - E2C_TIES[i]) < 5e-3


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("key", ["u8", "f32"])
@pytest.mark.parametrize("i", range(3))
def test_c2e_model_vs_reference_fixture(g, i, key, mode):
    h, w, F = M.C2E_SHAPES[i]
    cube, want = g["c2e_%d_%s_in" % (i, key)], g["c2e_%d_%s_%s" % (i, key, mode)]
    assert cube.shape[:2] == (F, 6 * F) and want.dtype == np.float64 and want.shape[:2] == (h, w)
    share = M.check(M.c2e(cube, h, w, ORDER[mode]), want, M.c2e_setup(cube, h, w), ORDER[mode], float(g["c2e_%d_eps" % i]),
                    "c2e %d %s %s" % (i, key, mode))
    if mode == "nearest":
        assert abs(share - C2E_TIES[i]) < 5e-3


def test_model_hazard_cases_are_present(g):
    """What the GPU cases are named for really happens on these shapes (read off the model's own coordinates)."""
    for i, (H, W, F) in enumerate(M.E2C_SHAPES):
        cx, cy = M.e2c_coords(H, W, F)
        up, down, back = cy[:, 4 * F:5 * F], cy[:, 5 * F:], cx[:, 2 * F:3 * F]
        if F % 2:                                                   # an odd face has a pixel on the pole itself
            assert (up < 0).any() and (down > H - 1).any()          # rows -1 -> H + 1 (wrap) and H: the pole rows
        assert (back < 1).any() and (back > W - 2).any()            # the B face holds both ends of the +-180 degree seam
    for i, (h, w, F) in enumerate(M.C2E_SHAPES):
        tp, cx, cy = M.c2e_coords(h, w, F)
        assert ((cx > F - 1) | (cy > F - 1)).mean() > 0.02          # taps in the appended rows / columns
        for f in range(6 if i < 2 else 4):                          # (the 31 x 56 caps stay inside the U face)
            assert ((tp == f) & ((cx > F - 1) | (cy > F - 1))).any(), (i, f)


# ------------------------------------------------------------------------------------------------ cube formats
def _cube(F=5, C=3, seed=0):
    return np.random.default_rng(seed).integers(0, 255, (F, 6 * F, C)).astype(np.uint8)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_format_helpers_round_trip(as_tensor):
    h = _cube()
    x = torch.from_numpy(h) if as_tensor else h
    eq = (lambda a, b: torch.equal(a, b)) if as_tensor else np.array_equal
    faces = P.cube_h2list(x)
    assert len(faces) == 6 and all(tuple(f.shape) == (5, 5, 3) for f in faces)
    assert eq(P.cube_list2h(faces), x)
    d = P.cube_h2dict(x)
    assert list(d) == ["F", "R", "B", "L", "U", "D"] and eq(d["L"], faces[3])
    assert eq(P.cube_dict2h(d), x)
    assert eq(P.cube_dict2h(d, face_k=["D", "U", "L", "B", "R", "F"]), P.cube_list2h(faces[::-1]))
    dice = P.cube_h2dice(x)
    assert tuple(dice.shape) == (15, 20, 3) and dice.dtype == x.dtype
    assert eq(P.cube_dice2h(dice), x)
    for fmt in ("horizon", "list", "dict", "dice"):
        assert eq(P.to_horizon(P.from_horizon(x, fmt), fmt), x)
    with pytest.raises(NotImplementedError):
        P.from_horizon(x, "cross")
    with pytest.raises(NotImplementedError):
        P.to_horizon(x, "cross")


def test_dice_layout_stated_directly():
    """U above F, D below it, L F R B along the middle row; R and B mirrored left-right, U up-down; corners zero."""
    h = _cube(F=4, C=1, seed=1)
    F_, R, B, L, U, D = (h[:, i * 4:(i + 1) * 4] for i in range(6))
    z = np.zeros((4, 4, 1), np.uint8)
    want = np.concatenate([np.concatenate([z, U[::-1], z, z], 1), np.concatenate([L, F_, R[:, ::-1], B[:, ::-1]], 1),
                           np.concatenate([z, D, z, z], 1)], 0)
    assert np.array_equal(P.cube_h2dice(h), want)


def test_fixture_dice_and_horizon_outputs_map_onto_each_other(g):
    for key in ("u8", "f32"):
        for mode in ORDER:
            hor, dice = g["e2c_1_%s_%s" % (key, mode)], g["e2c_1_%s_%s_dice" % (key, mode)]
            assert np.array_equal(P.cube_h2dice(hor), dice) and np.array_equal(P.cube_dice2h(dice), hor)
        assert np.array_equal(P.cube_dice2h(g["c2e_1_%s_in_dice" % key]), g["c2e_1_%s_in" % key])


# ------------------------------------------------------------------------------------------------ utils.pano
def test_cubemap_takes_the_four_formats():
    from panfusion_amd.utils.pano import Cubemap
    h = _cube()
    for fmt in ("horizon", "list", "dict", "dice"):
        assert np.array_equal(Cubemap(P.from_horizon(h, fmt), fmt).cubemap, h)
    with pytest.raises(NotImplementedError):
        Cubemap(h, "cross")
    with pytest.raises(AssertionError):
        Cubemap(h[:, :-1], "horizon")


def test_cubemap_from_mp3d_skybox(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from panfusion_amd.utils.pano import Cubemap
    rng = np.random.default_rng(2)
    folder = tmp_path / "scene0" / "matterport_skybox_images"
    folder.mkdir(parents=True)
    stored = [rng.integers(0, 255, (6, 6, 3)).astype(np.uint8) for _ in range(6)]
    for i, img in enumerate(stored):
        Image.fromarray(img).save(str(folder / ("view7_skybox%d_sami.png" % i)))
        (folder / ("view7_skybox%d_sami.png" % i)).rename(folder / ("view7_skybox%d_sami.jpg" % i))    # lossless bytes, the reference's name
    cm = Cubemap.from_mp3d_skybox(str(tmp_path), "scene0", "view7")
    up, left, front, right, back, down = stored                      # skybox0..5 = U L F R B D
    want = [front, right[:, ::-1], back[:, ::-1], left, np.rot90(up[::-1], 1), np.rot90(down, 1)]     # F R B L U D
    assert cm.cubemap.shape == (6, 36, 3) and cm.cubemap.dtype == np.uint8
    assert np.array_equal(cm.cubemap, np.concatenate(want, 1))


# ------------------------------------------------------------------------------------------------ refusals
def test_python_level_refusals():
    pano, cube = np.zeros((8, 16, 3), np.uint8), np.zeros((4, 24, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="unknown mode"):
        P.e2c(pano, 4, mode="bicubic")
    with pytest.raises(NotImplementedError, match="unknown mode"):
        P.c2e(cube, 8, 16, mode="bicubic", cube_format="horizon")
    with pytest.raises(NotImplementedError):
        P.e2c(pano, 4, cube_format="cross")
    with pytest.raises(NotImplementedError, match="unknown cube_format"):
        P.c2e(cube, 8, 16, cube_format="cross")
    with pytest.raises(AssertionError):
        P.c2e(cube, 8, 12, cube_format="horizon")                   # w % 8
    with pytest.raises(AssertionError):
        P.e2c(pano[..., 0], 4)                                      # [H, W]
    with pytest.raises(AssertionError):
        P.c2e(cube[..., 0], 8, 16, cube_format="horizon")
    with pytest.raises(AssertionError):
        P.c2e(cube[:, :-1], 8, 16, cube_format="horizon")           # not [w, 6w, C]
    with pytest.raises(TypeError):
        P.e2c(pano.astype(np.float64), 4)
    with pytest.raises(TypeError):
        P.c2e(cube.astype(np.float16), 8, 16, cube_format="horizon")
    with pytest.raises(TypeError):
        P.c2e(cube, 8, 16, cube_format="horizon", out_dtype=np.int32)
    with pytest.raises(TypeError):
        P.e2c_batch(torch.zeros(1, 8, 16, 3, dtype=torch.float64), 4)


def test_ceil_rows_follow_the_reference_expression():
    from panfusion_amd.external.py360convert.cube import facetype_ceil_rows
    for h, w, _ in M.C2E_SHAPES + ((1024, 2048, 0),):
        rows = facetype_ceil_rows(h, w)
        assert rows.dtype == np.intc and rows.shape == (w // 4,) and rows.min() >= 0 and rows.max() <= h // 2
        tp = M.facetype(h, w)
        q = (np.arange(w) - 3 * w // 8) % w % (w // 4)
        assert np.array_equal((tp == 4).sum(0), np.minimum(rows[q], h - rows[q]))     # U rows per column (D wins overlaps)
