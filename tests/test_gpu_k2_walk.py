"""The hypothesis walk of the exact K2 vector builds (k_reproject_st's full-tile builds; "k2_hyp_walk"): a workgroup scores 2 or 4 consecutive hypothesis
tiles of one frame on its pixel tile, loading and splitting the tile's coordinates once.

Every case runs the same call with "k2_hyp_walk" 1 and with the walk asked for, in one process, and wants the same bits in every output; the call at walk 1
is the one tests/test_gpu_k2_exact.py and tests/test_gpu_k2_full_tile.py pin to the oracle.  "k2_hyp_walk_last" tells the walk that ran: the plan shortens a
walk that would straddle a frame or the end of N (dsac_amd/csrc/k2_plan.h, k2_hyp_walk; its sweep is tests/test_k2_walk_plan_cpu.py).

Maps are implicit grids with W = 64.  The float cases force the <64 hypotheses, 256 cells> tile (k2_variant 85 with bit 28): 64 x 8 cells are two pixel tiles.
The 16-bit images and per-frame cameras accept no variant: they run on the <64, 64> tile the policy gives that map (eight pixel tiles, the same walk) and on
64 x 260, just above the policy's switch to <64, 256>."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAU, BETA = 10.0, 0.5
EXACT, GENERAL = 1 << 28, 1 << 30
VEC = "exact (vector build)"
W = 64
GUARD = 3  # rows behind the error images no launch may touch


def _defaults(e):
    for key, v in (("k2_variant", -1), ("k2_flags", 0), ("k2_exact_auto", 1), ("k2_f16_store", 1), ("pi_defer_tail", 0), ("k2_hyp_walk", 0)):
        e.set_option(key, v)


@pytest.fixture()
def eng(engine):
    _defaults(engine)
    yield engine
    engine.synchronize()
    _defaults(engine)


def _cam(H):
    return (525.0 * W / 640, 525.0 * W / 640, W / 2.0, H / 2.0)


_SCENES = {}


def _scene(synth, H, F, N):
    """F different frames of 64 x H cells, each under a camera of its own, and N hypotheses per frame around each frame's true pose: made once per shape"""
    key = (H, F, N)
    if key not in _SCENES:
        f0 = _cam(H)
        cams = np.array([(f0[0] * (1.0 + 0.05 * f), f0[1] * (1.0 + 0.05 * f), f0[2] + 1.5 * f, f0[3] - 1.0 * f) for f in range(F)], np.float32)
        frames = [synth.chess_like_frame(H, W, seed=5200 + 11 * H + f, cam=tuple(float(v) for v in cams[f]), grid_uv=True) for f in range(F)]
        rng = np.random.default_rng(300 + H + N)
        poses = np.concatenate([fr["gt_pose"][None] + rng.normal(size=(N, 6)) * np.array([0.02, 0.02, 0.02, 30.0, 30.0, 30.0]) for fr in frames])
        _SCENES[key] = dict(H=H, F=F, N=N, P=H * W, cams=cams, xyz=np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames])), poses=poses)
    return _SCENES[key]


def _set(eng, s, xyz=None, cams=False):
    xyz = s["xyz"] if xyz is None else xyz
    if cams:
        eng.set_frames(xyz, None, s["H"], W, s["cams"])
    elif s["F"] == 1:
        eng.set_frame(xyz[0], None, s["H"], W, tuple(float(v) for v in s["cams"][0]))
    else:
        eng.set_frames(xyz, None, s["H"], W, tuple(float(v) for v in s["cams"][0]))


def _run(eng, poses, P, walk, variant, flags=0, want=("err", "soft"), elem=None):
    """one dsac_reproject call; returns (err with its guard rows or None, soft or None, the walk that ran)"""
    n = len(poses)
    eng.set_option("k2_variant", variant)
    eng.set_option("k2_flags", flags | (EXACT if variant >= 0 else 0))
    eng.set_option("k2_hyp_walk", walk)
    buf = soft = None
    if "err" in want:
        buf = np.full((n + GUARD, P), 0x5A5A, np.uint16) if elem else np.full((n + GUARD, P), -7.0, np.float32)
    if "soft" in want:
        soft = np.full(n, -1.0)
    err = None if buf is None else buf[:n].view(np.float16) if elem == "f16" else buf[:n]
    eng.reproject(poses, err=err, soft=soft, tau=TAU, beta=BETA, elem=elem)
    assert eng.k2_form() == (VEC, 0)
    return buf, soft, eng.get_option("k2_hyp_walk_last")


def _same_as_walk_1(eng, poses, P, ask, expect, variant=85, **kw):
    """the call at walk 1 and at the walk asked for: the reported walks, equal bits in every output, untouched guard rows; returns walk 1's (err, soft)"""
    e1, s1, w1 = _run(eng, poses, P, 1, variant, **kw)
    ek, sk, wk = _run(eng, poses, P, ask, variant, **kw)
    assert (w1, wk) == (1, expect), "asked for a walk of %d on %d hypotheses: ran %d, expected %d" % (ask, len(poses), wk, expect)
    n = len(poses)
    if e1 is not None:
        bits = {2: np.uint16, 4: np.uint32}[e1.dtype.itemsize]
        fill = e1[n:].view(bits).copy()
        assert (fill == fill.flat[0]).all(), "walk 1 wrote behind row N"
        assert np.array_equal(ek[n:].view(bits), fill), "rows behind N were written"
        bad = np.argwhere(e1[:n].view(bits) != ek[:n].view(bits))
        assert bad.size == 0, "%d cells differ from walk 1, first (hypothesis, cell) %s" % (len(bad), tuple(bad[0]))
        assert (e1[:n].view(bits) != fill.flat[0]).all(), "a cell of the error images was never written"
    if s1 is not None:
        assert np.array_equal(s1.view(np.uint64), sk.view(np.uint64)), "soft differs from walk 1"
        assert (s1 >= 0.0).all()
    return e1, s1


MODES = [pytest.param(("err", "soft"), id="err+soft"), pytest.param(("err",), id="err"), pytest.param(("soft",), id="soft")]


# ---- whole walks: 1 x 128 at 2, 1 x 256 at 4 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", MODES)
@pytest.mark.parametrize("N, walk", [(128, 2), (256, 4), (256, 2)])
def test_one_whole_walk(eng, synth, N, walk, want):
    s = _scene(synth, 8, 1, N)
    _set(eng, s)
    _same_as_walk_1(eng, s["poses"], s["P"], walk, walk, want=want)


# ---- the legality rule ----------------------------------------------------------------------------------------------------------------------------------
def test_a_walk_that_would_pass_the_end_of_N_is_shortened(eng, synth):
    """192 hypotheses are three tiles: neither 4 nor 2 divides them"""
    s = _scene(synth, 8, 1, 192)
    _set(eng, s)
    _same_as_walk_1(eng, s["poses"], s["P"], 4, 1)
    _same_as_walk_1(eng, s["poses"], s["P"], 2, 1)


@pytest.mark.parametrize("ask", [2, 4])
def test_a_ragged_last_tile_falls_back(eng, synth, ask):
    """200 hypotheses: three whole tiles and one of 8"""
    s = _scene(synth, 8, 1, 200)
    _set(eng, s)
    _same_as_walk_1(eng, s["poses"], s["P"], ask, 1)


def test_an_unknown_walk_is_refused_by_name(eng):
    from dsac_amd import capi
    for bad in (3, 8, -1):
        with pytest.raises(capi.DsacError, match="k2_hyp_walk"):
            eng.set_option("k2_hyp_walk", bad)
    assert eng.get_option("k2_hyp_walk") == 0


# ---- frame batches, one camera and one set of coordinates per frame: a walk across a frame boundary would change results -------------------------------
@pytest.mark.parametrize("H", [8, 260])
@pytest.mark.parametrize("F, N, ask, expect", [(3, 128, 4, 2), (2, 256, 4, 4), (2, 256, 2, 2)])
def test_no_walk_straddles_a_frame(eng, synth, H, F, N, ask, expect):
    s = _scene(synth, H, F, N)
    _set(eng, s, cams=True)
    assert eng.get_option("frame_cams") == 1
    err, _ = _same_as_walk_1(eng, s["poses"], s["P"], ask, expect, variant=-1)
    # the frames differ: the same poses on another frame's rows give other images
    assert not np.array_equal(err[:N], err[N:2 * N])


# ---- tiles that leave the full-tile path inside a walk -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, walk", [(128, 2), (256, 4)])
def test_partial_last_pixel_tile(eng, synth, N, walk):
    """64 x 9: the third 256-cell tile holds one chunk and takes the general path, once per tile of the walk"""
    s = _scene(synth, 9, 1, N)
    _set(eng, s)
    _same_as_walk_1(eng, s["poses"], s["P"], walk, walk)


@pytest.mark.parametrize("N, walk", [(128, 2), (256, 4)])
def test_far_chunk_in_the_second_pixel_tile(eng, synth, N, walk):
    s = _scene(synth, 8, 1, N)
    xyz = s["xyz"].copy()
    xyz[0, 5 * W + 17, 0] = 70000.0  # |X| = 70 m: beyond the split's +-65.5 m
    _set(eng, s, xyz=xyz)
    far, _ = eng.k2_census(s["poses"])
    assert far >= 1
    _same_as_walk_1(eng, s["poses"], s["P"], walk, walk)


@pytest.mark.parametrize("N, walk", [(128, 2), (256, 4)])
def test_zero_depth_under_a_hypothesis_of_the_second_tile(eng, synth, N, walk):
    s = _scene(synth, 8, 1, N)
    xyz, poses = s["xyz"].copy(), s["poses"].copy()
    poses[64 + 3] = 0.0  # the zero pose: camera frame = scene frame ...
    cell = 2 * W + 41
    xyz[0, cell, 2] = 0.0  # ... so this cell has z == 0 exactly for hypothesis 67, in the walk's second tile
    _set(eng, s, xyz=xyz)
    err, soft = _same_as_walk_1(eng, poses, s["P"], walk, walk)
    assert np.isfinite(err[:N]).all() and np.isfinite(soft).all()


def test_the_general_path_walks_too(eng, synth):
    """"k2_flags" bit 30: every workgroup produces its tiles on the general path"""
    s = _scene(synth, 8, 1, 256)
    _set(eng, s)
    e0, s0 = _same_as_walk_1(eng, s["poses"], s["P"], 4, 4)
    e1, s1 = _same_as_walk_1(eng, s["poses"], s["P"], 4, 4, flags=GENERAL)
    assert np.array_equal(e0.view(np.uint32), e1.view(np.uint32)) and np.array_equal(s0.view(np.uint64), s1.view(np.uint64))


# ---- 16-bit error images --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("elem", ["f16", "bf16"])
@pytest.mark.parametrize("H", [8, 260])
def test_sixteen_bit_error_images(eng, synth, H, elem, layout):
    s = _scene(synth, H, 1, 256)
    _set(eng, s)
    eng.set_option("k2_f16_store", layout)
    for walk in (2, 4):
        _same_as_walk_1(eng, s["poses"], s["P"], walk, walk, variant=-1, elem=elem)
    _same_as_walk_1(eng, s["poses"], s["P"], 4, 4, variant=-1, elem=elem, want=("err",))


# ---- the fused scoring call with its tail deferred ----------------------------------------------------------------------------------------------------
def test_score_hypotheses_frames_with_the_tail_deferred(eng, synth):
    import torch
    dev = torch.device("cuda", 0)
    s = _scene(synth, 8, 2, 128)
    F, N, P = 2, 128, s["P"]
    xyz = torch.from_numpy(s["xyz"]).to(dev)
    out = []
    for walk in (1, 2):
        eng.set_frames(xyz, None, s["H"], W, tuple(float(v) for v in s["cams"][0]), borrow=True)
        eng.set_option("k2_variant", 85)
        eng.set_option("k2_flags", EXACT)
        eng.set_option("k2_hyp_walk", walk)
        eng.set_option("pi_defer_tail", 2)
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
        b = (z(F * N, 6), z(F * N, 4, dtype=torch.int32), z(F * N, dtype=torch.uint8), z(F * N), z(F * N), z(F), z(F, 6))
        err = torch.full((F * N + GUARD, P), -7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        eng.scoreHypothesesFrames(N, seed=77, tau=TAU, beta=BETA, scale=0.1, err=err[:F * N], out=b)
        eng.joinTail()
        eng.synchronize()
        assert eng.k2_form() == (VEC, 0) and eng.get_option("k2_hyp_walk_last") == walk
        eng.set_option("pi_defer_tail", 0)
        out.append([t.cpu().numpy() for t in b] + [err.cpu().numpy()])
    for a, k in zip(*out):
        assert np.array_equal(a.view(np.uint8), k.view(np.uint8))
    assert (out[0][-1][F * N:] == -7.0).all() and (out[0][-1][:F * N] != -7.0).all()
    assert out[0][3].max() > 0.0  # scores were written
    # leave a host frame behind: the borrowed device frame goes out of scope with this test
    _set(eng, _scene(synth, 8, 1, 128))
