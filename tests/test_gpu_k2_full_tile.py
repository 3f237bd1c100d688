"""The full-tile path of the exact K2 vector builds (k_reproject_st, EXF != 0, ANY == 0) against the general path of the same kernel.

A tile takes the full-tile path when its hypothesis tile is whole, every chunk lies inside the map and no chunk holds a coordinate beyond the split's range;
"k2_flags" bit 30 sends every tile down the general path.  Every case runs the same call twice in one process, default and bit 30, and asks for the same
bits in the error images and in the soft-inlier sums, and for the stated 1e-3 px against the oracle.  The partial sums themselves cannot be read through the
API: `soft` is their sum in double in a fixed order (exact for the at most eight rows of these maps), and case (a) adds a one-tile map on which `soft` IS the
tile's partial sum.

Maps are implicit grids with W = 64 (a chunk is one row).  Two tiles: the <64 hypotheses, 64 cells> tile the auto policy gives maps of this size, and the
bench shape's <64, 256> tile (k2_variant 85 with bit 28; the 16-bit images and per-frame cameras accept no variant, so their <64, 256> case is a map just
above the policy's 16 384-cell switch)."""

import numpy as np
import pytest

from conftest import excl_clamp_edge, margin

pytestmark = pytest.mark.gpu

TAU, BETA, CLAMP = 10.0, 0.5, 100.0
EXACT, GENERAL = 1 << 28, 1 << 30
VEC = "exact (vector build)"
W = 64
TILES = [pytest.param(-1, id="tile 64x64"), pytest.param(85, id="tile 64x256")]


def _defaults(e):
    for key, v in (("k2_variant", -1), ("k2_flags", 0), ("k2_exact_auto", 1), ("k2_f16_store", 1), ("pi_defer_tail", 0)):
        e.set_option(key, v)


@pytest.fixture()
def eng(engine):
    _defaults(engine)
    yield engine
    _defaults(engine)


def _cam(H):
    """525 px at 640 columns scaled to the map, the principal point at its centre"""
    return (525.0 * W / 640, 525.0 * W / 640, W / 2.0, H / 2.0)


_SCENES = {}


def _scene(synth, H, F, N):
    """F frames of 64 x H cells and N hypotheses per frame around each frame's true pose: made once per shape, shared and left unchanged"""
    key = (H, F, N)
    if key not in _SCENES:
        frames = [synth.chess_like_frame(H, W, seed=4100 + 7 * H + f, cam=_cam(H), grid_uv=True) for f in range(F)]
        rng = np.random.default_rng(900 + H)
        poses = np.concatenate([fr["gt_pose"][None] + rng.normal(size=(N, 6)) * np.array([0.02, 0.02, 0.02, 30.0, 30.0, 30.0]) for fr in frames])
        _SCENES[key] = dict(H=H, F=F, N=N, P=H * W, frames=frames, xyz=np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames])), poses=poses,
                            uv=synth.pixel_grid(H, W, H, W))
    return _SCENES[key]


def _set(eng, s, xyz=None, cams=None):
    xyz = s["xyz"] if xyz is None else xyz
    cam = _cam(s["H"]) if cams is None else cams
    if s["F"] == 1 and cams is None:
        eng.set_frame(xyz[0], None, s["H"], W, cam)
    else:
        eng.set_frames(xyz, None, s["H"], W, cam)


def _both_paths(eng, poses, P, variant=-1, dtype=np.float32, elem=None):
    """the call on the default path choice and with every tile on the general path; asserts equal bits, returns the default's (err, soft)"""
    out = []
    for flags in (0, GENERAL):
        eng.set_option("k2_variant", variant)
        eng.set_option("k2_flags", flags | (EXACT if variant >= 0 else 0))
        err = np.full((len(poses), P), 0x5A5A, np.uint16) if dtype == np.uint16 else np.full((len(poses), P), -7.0, dtype)
        soft = np.full(len(poses), -1.0)
        eng.reproject(poses, err=err, soft=soft, tau=TAU, beta=BETA, elem=elem)
        assert eng.k2_form() == (VEC, 0)
        out.append((err, soft))
    _defaults(eng)
    (e0, s0), (e1, s1) = out
    bits = {2: np.uint16, 4: np.uint32}[e0.dtype.itemsize]
    bad = np.argwhere(e0.view(bits) != e1.view(bits))
    assert bad.size == 0, "%d cells differ between the two paths, first (hypothesis, cell) %s" % (len(bad), tuple(bad[0]))
    assert np.array_equal(s0.view(np.uint64), s1.view(np.uint64)), "soft differs between the two paths"
    return e0, s0


def _against_oracle(orc, s, err, soft, what, xyz=None, poses=None, cams=None, skip=None):
    """every frame's rows against the oracle under its camera: 1e-3 px on every cell off the clamp edge (skip: a mask of cells left out), the sums to 2e-6"""
    xyz = s["xyz"] if xyz is None else xyz
    poses = s["poses"] if poses is None else poses
    N, worst, worst_s = s["N"], 0.0, 0.0
    for f in range(s["F"]):
        sl = slice(f * N, (f + 1) * N)
        cam = _cam(s["H"]) if cams is None else tuple(float(v) for v in cams[f])
        ref = orc.get_diff_maps(poses[sl], xyz[f], s["uv"], s["H"], W, cam)
        m = excl_clamp_edge(err[sl], ref, CLAMP)
        if skip is not None:
            m &= ~skip[f][None, :]
        assert m.any()
        worst = max(worst, float(np.abs(err[sl] - ref)[m].max()))
        if soft is not None and skip is None:
            sr = orc.soft_inlier(ref, TAU, BETA)
            worst_s = max(worst_s, float(np.abs(soft[sl] - sr).max() / max(1.0, sr.max())))
    margin("a3", "K2 full-tile path, %s: max |err - oracle| px" % what, worst, 1e-3)
    if soft is not None and skip is None:
        assert worst_s <= 2e-6, worst_s
    return worst


# ---- (a) every tile is full ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", TILES)
def test_every_tile_full(eng, orc, synth, variant):
    s = _scene(synth, 8, 2, 128)
    _set(eng, s)
    err, soft = _both_paths(eng, s["poses"], s["P"], variant)
    _against_oracle(orc, s, err, soft, "2 x 128 x 64x8, every tile full (k2_variant %d)" % variant)
    # one pixel tile: soft[h] is that tile's partial sum
    one = _scene(synth, 4 if variant == 85 else 1, 1, 128)
    _set(eng, one)
    e1, s1 = _both_paths(eng, one["poses"], one["P"], variant)
    assert np.array_equal(s1, s1.astype(np.float32).astype(np.float64)), "a one-tile map: soft is one fp32 partial sum"


# ---- (b) a full and a ragged hypothesis tile in one launch --------------------------------------------------------------------------------
# N = 77: the rows of partial sums start off the 16-byte grid, and the full tile writes its four sums per lane as one 16-byte store
@pytest.mark.parametrize("N", [80, 77])
@pytest.mark.parametrize("variant", TILES)
def test_full_and_ragged_hypothesis_tile(eng, orc, synth, variant, N):
    s = _scene(synth, 12, 1, N)
    _set(eng, s)
    err, soft = _both_paths(eng, s["poses"], s["P"], variant)
    _against_oracle(orc, s, err, soft, "%d x 64x12, a full and a ragged hypothesis tile (k2_variant %d)" % (N, variant))


# ---- (c) a full pixel tile and a last tile of one chunk -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", TILES)
def test_last_pixel_tile_of_one_chunk(eng, orc, synth, variant):
    s = _scene(synth, 5, 2, 128)
    _set(eng, s)
    err, soft = _both_paths(eng, s["poses"], s["P"], variant)
    _against_oracle(orc, s, err, soft, "2 x 128 x 64x5, the last 256-cell tile holds one chunk (k2_variant %d)" % variant)


# ---- (d) one far cell: its tile goes general, the others stay full ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", TILES)
def test_one_far_cell(eng, orc, synth, variant):
    s = _scene(synth, 8, 2, 128)
    xyz = s["xyz"].copy()
    cell = 5 * W + 17
    xyz[1, cell, 0] = 70000.0  # |X| = 70 m in frame 1: beyond the split's +-65.5 m
    _set(eng, s, xyz=xyz)
    far, _ = eng.k2_census(s["poses"])
    assert far >= 1
    err, soft = _both_paths(eng, s["poses"], s["P"], variant)
    # the far cell's chunk takes the fp32 transform: the stated 1e-3 px holds for the cells in range
    skip = np.zeros((2, s["P"]), bool)
    skip[1, (cell // 64) * 64:(cell // 64 + 1) * 64] = True
    _against_oracle(orc, s, err, None, "one cell at |X| = 70 m, the cells of every other chunk (k2_variant %d)" % variant, xyz=xyz, skip=skip)


# ---- (e) a cell on a hypothesis's camera plane: the exact-z redo inside the full-tile path --------------------------------------------------
@pytest.mark.parametrize("variant", TILES)
def test_cell_on_the_camera_plane(eng, orc, synth, variant):
    s = _scene(synth, 8, 2, 128)
    xyz, poses = s["xyz"].copy(), s["poses"].copy()
    poses[3] = 0.0             # the zero pose: camera frame = scene frame ...
    cell = 2 * W + 41
    xyz[0, cell, 2] = 0.0      # ... so this cell of frame 0 has z == 0 for hypothesis 3
    _set(eng, s, xyz=xyz)
    err, soft = _both_paths(eng, poses, s["P"], variant)
    assert np.isfinite(err).all() and np.isfinite(soft).all()
    _against_oracle(orc, s, err, soft, "one cell on the camera plane of a hypothesis (k2_variant %d)" % variant, xyz=xyz, poses=poses)
    ref = orc.get_diff_maps(poses[3:4], xyz[0], s["uv"], s["H"], W, _cam(s["H"]))
    assert abs(float(err[3, cell]) - float(ref[0, cell])) <= 1e-3 or (err[3, cell] >= CLAMP - 1e-3 and ref[0, cell] >= CLAMP - 1e-3)


# ---- (f) 16-bit error images -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("elem", ["f16", "bf16"])
@pytest.mark.parametrize("H", [8, 260])  # 64 x 260 = 16 640 cells: above the switch to the <64, 256> tile, 65 full tiles
def test_sixteen_bit_error_images(eng, orc, synth, H, elem, layout):
    s = _scene(synth, H, 2, 128)
    _set(eng, s)
    e32, s32 = _both_paths(eng, s["poses"], s["P"])
    eng.set_option("k2_f16_store", layout)
    out = []
    for flags in (0, GENERAL):
        eng.set_option("k2_flags", flags)
        e16, s16 = np.full((len(s["poses"]), s["P"]), 0x5A5A, np.uint16), np.full(len(s["poses"]), -1.0)
        eng.reproject(s["poses"], err=e16.view(np.float16) if elem == "f16" else e16, soft=s16, tau=TAU, beta=BETA, elem=elem)
        assert eng.k2_form() == (VEC, 0)
        out.append((e16, s16))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64))
    assert np.array_equal(out[0][1].view(np.uint64), s32.view(np.uint64)), "soft of the 16-bit call is the float call's"
    if elem == "f16":
        assert np.array_equal(out[0][0], e32.astype(np.float16).view(np.uint16))
    else:
        b = e32.view(np.uint32).astype(np.uint64)
        assert np.array_equal(out[0][0], ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16))  # round to nearest even; no NaN among clamped errors
    if elem == "f16" and layout == 1:
        _against_oracle(orc, s, e32, s32, "the float images the 16-bit ones round, 2 x 128 x 64x%d" % H)


# ---- (g) one camera per frame ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 260])
def test_one_camera_per_frame(eng, orc, synth, H):
    s = _scene(synth, H, 2, 128)
    f0 = _cam(H)
    cams = np.array([f0, (f0[0] * 1.11, f0[1] * 1.11, f0[2] + 3.0, f0[3] - 2.0)], np.float32)
    frames = [synth.chess_like_frame(H, W, seed=4100 + 7 * H + f, cam=tuple(float(v) for v in cams[f]), grid_uv=True) for f in range(2)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    rng = np.random.default_rng(77 + H)
    poses = np.concatenate([fr["gt_pose"][None] + rng.normal(size=(128, 6)) * np.array([0.02, 0.02, 0.02, 30.0, 30.0, 30.0]) for fr in frames])
    _set(eng, s, xyz=xyz, cams=cams)
    assert eng.get_option("frame_cams") == 1
    err, soft = _both_paths(eng, poses, s["P"])
    _against_oracle(orc, s, err, soft, "one camera per frame, 2 x 128 x 64x%d" % H, xyz=xyz, poses=poses, cams=cams)


# ---- (h) 640 x 480: the shape at which a first build of the <64, 64> tile stored wrong rows ----------------------------------------------------
# Nothing stalls a wave behind its stores in the full-tile path, and that build let a vector instruction write a store's data register directly behind the
# store: a few chunks of a launch, other ones every run, held the new value in lanes 12-15 -- only with 4 800 waves in flight, never on the small maps above.
# Bits only (the oracle comparison at this shape is tests/test_gpu_k2_exact.py's): default against the general path, which has never shown it; device buffers.
@pytest.mark.parametrize("what", ["tile 64x64", "tile 64x256", "f16", "bf16"])
def test_both_paths_at_640x480(eng, synth, what):
    import torch
    dev = torch.device("cuda", 0)
    H, Wd, N = 480, 640, 64
    fr = synth.chess_like_frame(H, Wd, seed=77, grid_uv=True)
    eng.set_frame(fr["xyz"], None, H, Wd, fr["cam"])
    poses = fr["gt_pose"][None] + np.random.default_rng(5).normal(size=(N, 6)) * np.array([0.02, 0.02, 0.02, 30.0, 30.0, 30.0])
    variant = {"tile 64x64": 94, "tile 64x256": 85}.get(what, -1)
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}.get(what, torch.float32)
    out = []
    for flags in (0, GENERAL):
        eng.set_option("k2_variant", variant)
        eng.set_option("k2_flags", flags | (EXACT if variant >= 0 else 0))
        err = torch.full((N, H * Wd), -7.0, dtype=dt, device=dev)
        soft = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
        for _ in range(3):  # the fault was sporadic: three launches each
            eng.reproject(poses, N=N, err=err, soft=soft, tau=TAU, beta=BETA)
        eng.synchronize()
        assert eng.k2_form() == (VEC, 0)
        out.append((err, soft))
    _defaults(eng)
    bits = torch.int32 if dt == torch.float32 else torch.int16
    differ = int((out[0][0].view(bits) != out[1][0].view(bits)).sum())
    assert differ == 0, "%d cells differ between the two paths" % differ
    assert torch.equal(out[0][1].view(torch.int64), out[1][1].view(torch.int64)), "soft differs between the two paths"
