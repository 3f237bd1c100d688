"""K2's exact-transform form on ANY map (k2_flags bit 29, and the auto policy): maps whose cell count is not a multiple of 4 and buffers off the 16-byte grid
take the any-map build of k_reproject_st -- the same arithmetic per cell as the vector build, bit for bit on the same cells -- instead of the fp32 fallback of
rounds 2-5; dsac_get_option("k2_form_last" / "k2_form_why_last") tells which form a launch took, dsac_k2_range_census counts what the exact form degrades on.
Every bound here is the stated one (1e-3 px per cell, 1e-4 on the softmax weights of a tie) or the bound the vector form's own tests assert
(tests/test_gpu_k2_exact.py: scores within 2e-6 / 2e-7 relative)."""
import numpy as np
import pytest

from conftest import excl_clamp_edge, margin

pytestmark = pytest.mark.gpu

H, W = 480, 640
P = H * W
TAU, BETA, SCALE, CLAMP = 10.0, 0.5, 0.1, 100.0
EXACT, EXACT_ANY, PRECISE = 1 << 28, 1 << 29, 1 << 25
VEC, ANY = "exact (vector build)", "exact (any-map build)"


def _defaults(e):
    e.set_option("k2_variant", -1)
    e.set_option("k2_flags", 0)
    e.set_option("k2_exact_auto", 1)


@pytest.fixture()
def eng(engine):
    _defaults(engine)
    yield engine
    _defaults(engine)


def near_tie_pairs(soft_ref):
    order = np.argsort(-soft_ref)
    return [(order[a], order[b]) for a in range(len(order)) for b in range(a + 1, len(order)) if soft_ref[order[a]] - soft_ref[order[b]] <= 0.05 * soft_ref.max()]


# ---- 1. the form report -----------------------------------------------------------------------------------------------------------------
def test_form_report(orc, synth):
    import dsac_amd
    from dsac_amd import capi
    with dsac_amd.Engine(0) as e:
        assert e.k2_form() == ("none", 0)
        fr = synth.chess_like_frame(H, W, seed=2305)
        e.set_frame(fr["xyz"], None, H, W, fr["cam"])
        poses, _, _ = e.sample(128, seed=4711, thr=10.0, max_tries=1 << 16)
        assert e.k2_form() == ("none", 0)  # K1 is no K2 launch
        soft = np.zeros(128)
        e.reproject(poses, soft=soft)
        assert e.k2_form() == (VEC, 0)
        e.set_option("k2_exact_auto", 0)
        e.reproject(poses, soft=soft)
        name, why = e.k2_form()
        assert name.startswith("fp32") and why == capi.DSAC_K2_WHY_AUTO_OFF
        e.set_option("k2_exact_auto", 1)
        e.set_option("k2_flags", PRECISE)
        e.reproject(poses, soft=soft)
        assert e.k2_form() == ("precise", capi.DSAC_K2_WHY_FORCED)
        e.set_option("k2_flags", 0)
        e.set_option("k2_variant", 42)
        e.reproject(poses, soft=soft)
        assert e.k2_form() == ("fp32 mfma", capi.DSAC_K2_WHY_FORCED)
        e.set_option("k2_variant", -1)
        # a focal length the split records do not take
        cam = (1100.0, 1100.0, 320.0, 240.0)
        ff = synth.chess_like_frame(H, W, seed=2305, cam=cam)
        e.set_frame(ff["xyz"], None, H, W, cam)
        pf, _, _ = e.sample(128, seed=4711, thr=10.0, max_tries=1 << 16)
        e.reproject(pf, soft=soft)
        name, why = e.k2_form()
        assert name.startswith("fp32") and why == capi.DSAC_K2_WHY_FOCAL
        e.set_option("k2_flags", EXACT_ANY)
        with pytest.raises(capi.DsacError):
            e.reproject(pf, soft=soft)
        assert e.k2_form()[0].startswith("fp32")  # the report is of the last launch that went out
        e.set_option("k2_flags", 0)
        # 53 x 37: an odd cell count
        fo = synth.chess_like_frame(37, 53, seed=5, grid_uv=True)
        e.set_frame(fo["xyz"], None, 37, 53, fo["cam"])
        po, _, _ = e.sample(64, seed=1, thr=10.0, max_tries=1 << 16)
        eo = np.zeros((64, 37 * 53), np.float32)
        e.reproject(po, err=eo)
        assert e.k2_form() == (ANY, 0)
        e.set_option("k2_flags", EXACT_ANY)
        eo2 = np.zeros_like(eo)
        e.reproject(po, err=eo2)
        assert e.k2_form() == (ANY, 0)
        assert np.array_equal(eo, eo2)
        ref = orc.get_diff_maps(po, fo["xyz"], fo["uv"], 37, 53, fo["cam"])
        m = excl_clamp_edge(eo, ref, CLAMP)
        assert np.abs(eo - ref)[m].max() <= 1e-3
        e.set_option("k2_flags", EXACT)  # bit 28 names the vector build: still an error here
        with pytest.raises(capi.DsacError):
            e.reproject(po, err=eo2)
        # bit 29 with one of the vector build's tile / tail trades is an error where only the any-map build fits: never another arithmetic under that name
        e.set_option("k2_flags", EXACT_ANY)
        e.set_option("k2_variant", 84)
        with pytest.raises(capi.DsacError):
            e.reproject(po, err=eo2)
        e.set_option("k2_variant", -1)
        # bit 29 on a vector map is the vector build
        e.set_frame(fr["xyz"], None, H, W, fr["cam"])
        e.reproject(poses, soft=soft)
        assert e.k2_form() == (VEC, 0)
        e.set_option("k2_variant", 84)
        e.reproject(poses, soft=soft)
        assert e.k2_form() == (VEC, 0)
        e.set_option("k2_variant", -1)
        # get_option returns what set_option stored
        for key, vals in (("k2_variant", (42, -1)), ("k2_flags", (EXACT_ANY | 1, 0)), ("k2_exact_auto", (0, 1)), ("pi_defer_tail", (2, 1, 0)), ("k2_order", (0, 1)),
                          ("seed_stride", (3, 1)), ("k6_waves", (4, 0))):
            for v in vals:
                e.set_option(key, v)
                assert e.get_option(key) == v
        with pytest.raises(capi.DsacError):
            e.get_option("no_such_key")


# ---- 2. one arithmetic, two builds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 200])
def test_the_two_builds_agree_bit_for_bit(eng, synth, N):
    """The form is a property of the arithmetic, not of the buffer: the same frame and poses through 16-byte-aligned buffers (vector build) and through
    buffers 4 / 8 bytes off (any-map build) give the same error images and soft sums bit for bit; a map one cell short gives the same cells."""
    import torch
    dev = torch.device("cuda", 0)
    fr = synth.chess_like_frame(H, W, seed=2305)
    cam = fr["cam"]
    uv_h = synth.pixel_grid(H, W)
    xyz_buf = torch.zeros(P * 3 + 4, dtype=torch.float32, device=dev)
    uv_buf = torch.zeros(P * 2 + 4, dtype=torch.float32, device=dev)
    xyz_al = torch.from_numpy(fr["xyz"].reshape(-1)).to(dev)
    uv_al = torch.from_numpy(np.ascontiguousarray(uv_h).reshape(-1)).to(dev)
    xyz_off, uv_off = xyz_buf[1:1 + P * 3], uv_buf[2:2 + P * 2]
    xyz_off.copy_(xyz_al)
    uv_off.copy_(uv_al)
    assert xyz_al.data_ptr() % 16 == 0 and uv_al.data_ptr() % 16 == 0 and xyz_off.data_ptr() % 16 == 4 and uv_off.data_ptr() % 16 == 8
    err_buf = torch.zeros(N * P + 4, dtype=torch.float32, device=dev)
    err_full = torch.zeros(N * P, dtype=torch.float32, device=dev)
    soft_a, soft_b = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    # aligned run; the poses are sampled once, on the aligned frame
    eng.set_frame(xyz_al, uv_al, H, W, cam, borrow=True)
    poses, _, _ = eng.sample(N, seed=4711, thr=10.0, max_tries=1 << 16)
    eng.reproject(poses, err=err_full, soft=soft_a, tau=TAU, beta=BETA)
    eng.synchronize()
    assert eng.k2_form() == (VEC, 0)
    # offset run: err + 4 bytes, xyz + 4 bytes, uv + 8 bytes
    err_off = err_buf[1:1 + N * P]
    assert err_off.data_ptr() % 16 == 4
    eng.set_frame(xyz_off, uv_off, H, W, cam, borrow=True)
    eng.reproject(poses, err=err_off, soft=soft_b, tau=TAU, beta=BETA)
    eng.synchronize()
    assert eng.k2_form() == (ANY, 0)
    assert torch.equal(err_off, err_full)
    assert torch.equal(soft_a, soft_b)
    assert float(err_buf[0].item()) == 0.0 and float(err_buf[1 + N * P:].abs().max().item()) == 0.0  # nothing written beside the images
    # the implicit grid (a map width of 64 k: the positions come from scalar registers) with only err off the 16-byte grid
    eng.set_frame(xyz_al, None, H, W, cam, borrow=True)
    err_buf.zero_()
    soft_b.zero_()
    torch.cuda.synchronize()
    eng.reproject(poses, err=err_off, soft=soft_b, tau=TAU, beta=BETA)
    eng.synchronize()
    assert eng.k2_form() == (ANY, 0)
    assert torch.equal(err_off, err_full) and torch.equal(soft_a, soft_b)
    # one cell short: 307 199 = 97 x 3167 cells (odd), sampled positions; every row starts on another alignment
    P1 = P - 1
    assert 97 * 3167 == P1
    xyz_t, uv_t = xyz_al[:P1 * 3], uv_al[:P1 * 2]
    err_t = err_buf[:N * P1]
    err_buf.zero_()
    torch.cuda.synchronize()
    eng.set_frame(xyz_t, uv_t, 97, 3167, cam, borrow=True)
    eng.reproject(poses, err=err_t, tau=TAU, beta=BETA)
    eng.synchronize()
    assert eng.k2_form() == (ANY, 0)
    assert torch.equal(err_t.view(N, P1), err_full.view(N, P)[:, :P1])
    assert float(err_buf[N * P1:].abs().max().item()) == 0.0
    # two more entry points on the truncated map: the same kernel, the same images
    del err_full
    f64 = dict(dtype=torch.float64, device=dev)
    out = (torch.zeros(N, 6, **f64), torch.zeros(N, 4, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev), torch.zeros(N, **f64),
           torch.zeros(N, **f64), torch.zeros(1, **f64), torch.zeros(6, **f64))
    err_s = torch.zeros(N * P1, dtype=torch.float32, device=dev)
    eng.scoreHypotheses(N, seed=4711, thr=10.0, max_tries=1 << 16, tau=TAU, beta=BETA, err=err_s, out=out)
    eng.synchronize()
    assert eng.k2_form() == (ANY, 0)
    err_buf.zero_()
    torch.cuda.synchronize()
    eng.reproject(out[0], N=N, err=err_t, soft=soft_b, tau=TAU, beta=BETA)
    eng.synchronize()
    assert torch.equal(err_t, err_s) and torch.equal(soft_b, out[3])
    p2 = (torch.zeros(N, 6, **f64), torch.zeros(N, 4, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev))
    err_s.zero_()
    soft_a.zero_()
    torch.cuda.synchronize()
    eng.processImagesBegin(N, err_s, seed=4711, thr=10.0, max_tries=1 << 16, tau=TAU, beta=BETA, soft=soft_a, out=p2)
    eng.synchronize()
    assert eng.k2_form() == (ANY, 0)
    assert torch.equal(p2[0], out[0]) and torch.equal(err_s, err_t) and torch.equal(soft_a, soft_b)


# ---- 3. the stated tolerances on maps the vector kernels cannot read, default options -----------------------------------------------------
@pytest.mark.parametrize("h,w,N,sampled", [(37, 53, 256, False), (41, 41, 77, True), (41, 41, 256, True), (37, 50, 256, False), (7, 5, 64, True), (7, 5, 256, False)])
def test_small_maps_hold_the_tolerances(eng, orc, synth, h, w, N, sampled):
    fr = synth.chess_like_frame(h, w, seed=5, grid_uv=True)
    eng.set_frame(fr["xyz"], fr["uv"] if sampled else None, h, w, fr["cam"])
    poses, _, _ = eng.sample(N, seed=4711, thr=10.0, max_tries=1 << 16)
    err, soft = np.zeros((N, h * w), np.float32), np.zeros(N)
    eng.reproject(poses, err=err, soft=soft, tau=TAU, beta=BETA)
    assert eng.k2_form() == (ANY if (h * w) % 4 else VEC, 0)
    if h * w == 35:
        # P3P on 35 cells returns poses outside the split records' range (|t_z| > 131 m): the any-map build sends their groups through the fp32 transform
        assert eng.k2_census(poses)[1] > 0
    ref = orc.get_diff_maps(poses, fr["xyz"], fr["uv"], h, w, fr["cam"])
    m = excl_clamp_edge(err, ref, CLAMP)
    margin("a3", "K2 any-map build, default options (%dx%d, N = %d): max |err - oracle| px" % (w, h, N), np.abs(err - ref)[m].max() if m.any() else 0.0, 1e-3)
    sr = orc.soft_inlier(ref, TAU, BETA)
    margin("north*", "K2 any-map build on small maps: soft-inlier scores, max |score - oracle| / max(1, largest score)", np.abs(soft - sr).max() / max(1.0, sr.max()), 2e-6,
           stated=1e-4)
    # soft sums alone (no error images): the same numbers
    soft2 = np.zeros(N)
    eng.reproject(poses, soft=soft2, tau=TAU, beta=BETA)
    assert np.array_equal(soft, soft2)


@pytest.mark.parametrize("seed", [2305, 2306, 2307])
def test_641x479_cells_scores_and_ties(eng, orc, synth, seed):
    """641 x 479 = 307 039 cells (odd), implicit grid of a width that is no multiple of 64, default options: every cell within the stated 1e-3 px, scores within
    2e-7 relative, and the near-tie weight error a tenth of the fp32 form's on the same poses; its absolute value is recorded against the stated 1e-4."""
    h, w = 479, 641
    fr = synth.chess_like_frame(h, w, seed=seed, grid_uv=True)
    eng.set_frame(fr["xyz"], None, h, w, fr["cam"])
    poses, _, _ = eng.sample(256, seed=4711, thr=10.0, max_tries=1 << 16)
    err, soft = np.zeros((256, h * w), np.float32), np.zeros(256)
    eng.reproject(poses, err=err, soft=soft, tau=TAU, beta=BETA)
    assert eng.k2_form() == (ANY, 0)
    ref = orc.get_diff_maps(poses, fr["xyz"], fr["uv"], h, w, fr["cam"])
    m = excl_clamp_edge(err, ref, CLAMP)
    d = np.abs(err - ref)
    d[~m] = 0
    margin("a3", "K2 any-map build, residuals over ALL cells of 256 x 641x479: max |err - oracle| px", d.max(), 1e-3)
    assert int((d > 1e-3).sum()) == 0
    soft_ref = orc.soft_inlier(ref, TAU, BETA)
    dsv = soft - soft_ref
    margin("north*", "K2 any-map build at 641x479: soft-inlier scores, max |score - oracle| relative to the largest score", np.abs(dsv).max() / max(1.0, soft_ref.max()), 2e-7,
           stated=1e-4)
    pairs = near_tie_pairs(soft_ref)
    assert len(pairs) >= 100
    tie = 0.25 * SCALE * max(abs(dsv[i] - dsv[j]) for i, j in pairs)
    eng.set_option("k2_exact_auto", 0)
    soft_f = np.zeros(256)
    eng.reproject(poses, soft=soft_f, tau=TAU, beta=BETA)
    assert eng.k2_form()[0].startswith("fp32")
    eng.set_option("k2_exact_auto", 1)
    tie_f = 0.25 * SCALE * max(abs((soft_f - soft_ref)[i] - (soft_f - soft_ref)[j]) for i, j in pairs)
    print("641x479 seed %d near-tie weight error: any-map exact %.2e, fp32 %.2e" % (seed, tie, tie_f))
    margin("a4", "K2 any-map build at 641x479: near-tie weight error of UNRELATED hypotheses, asserted against a tenth of the fp32 form's on the same poses", tie, 0.1 * tie_f,
           stated=1e-4)
    assert tie < 0.1 * tie_f


@pytest.mark.parametrize("seed", [2305, 2306, 2307])
def test_ties_on_the_truncated_map_hold_the_stated_bound(eng, orc, synth, seed):
    """307 199 cells (640 x 480 less one): the arithmetic of the vector form, whose margin against the stated 1e-4 is known (5.5-8.3e-5); one cell cannot move it."""
    P1 = P - 1
    fr = synth.chess_like_frame(H, W, seed=seed)
    xyz, uv, cam = np.ascontiguousarray(fr["xyz"][:P1]), np.ascontiguousarray(synth.pixel_grid(H, W)[:P1]), fr["cam"]
    eng.set_frame(xyz, uv, 97, 3167, cam)
    poses, _, _ = eng.sample(256, seed=4711, thr=10.0, max_tries=1 << 16)
    soft = np.zeros(256)
    eng.reproject(poses, soft=soft, tau=TAU, beta=BETA)
    assert eng.k2_form() == (ANY, 0)
    ref = orc.get_diff_maps(poses, xyz, uv, 97, 3167, cam)
    soft_ref = orc.soft_inlier(ref, TAU, BETA)
    dsv = soft - soft_ref
    pairs = near_tie_pairs(soft_ref)
    assert len(pairs) >= 100
    tie = 0.25 * SCALE * max(abs(dsv[i] - dsv[j]) for i, j in pairs)
    margin("a4", "K2 any-map build, 307 199 cells: softmax-weight error in a tie of two UNRELATED hypotheses, scale 0.1 -- 0.25 x scale x max |d_i - d_j|", tie, 1e-4)


def test_a_frame_batch_of_641x479(eng, orc, synth):
    """4 frames of 641 x 479 through set_frames / scoreHypothesesFrames: frame f starts 307 039 x 12 bytes further on, so the frames differ in alignment."""
    import torch
    dev = torch.device("cuda", 0)
    h, w, F, N = 479, 641, 4, 256
    Pm = h * w
    frames = [synth.chess_like_frame(h, w, seed=2305 + f, grid_uv=True) for f in range(F)]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))).to(dev)
    cam = frames[0]["cam"]
    eng.set_frames(xyz, None, h, w, cam, borrow=True)
    f64 = dict(dtype=torch.float64, device=dev)
    err = torch.zeros(F * N, Pm, dtype=torch.float32, device=dev)
    out = (torch.zeros(F * N, 6, **f64), torch.zeros(F * N, 4, dtype=torch.int32, device=dev), torch.zeros(F * N, dtype=torch.uint8, device=dev), torch.zeros(F * N, **f64),
           torch.zeros(F * N, **f64), torch.zeros(F, **f64), torch.zeros(F, 6, **f64))
    eng.scoreHypothesesFrames(N, seed=4711, thr=10.0, max_tries=1 << 16, tau=TAU, beta=BETA, err=err, out=out)
    eng.synchronize()
    assert eng.k2_form() == (ANY, 0)
    ph, sf = out[0].cpu().numpy(), out[3].cpu().numpy()
    f = 3
    got = err[f * N:(f + 1) * N].cpu().numpy()
    ref = orc.get_diff_maps(ph[f * N:(f + 1) * N], frames[f]["xyz"], frames[f]["uv"], h, w, cam)
    m = excl_clamp_edge(got, ref, CLAMP)
    d = np.abs(got - ref)
    d[~m] = 0
    margin("a3", "K2 any-map build, frame batch 4 x 256 x 641x479, ALL rows of one frame: max |err - oracle| px", d.max(), 1e-3)
    sr = orc.soft_inlier(ref, TAU, BETA)
    margin("north*", "K2 any-map build, frame batch of 641x479: soft-inlier scores of a whole frame, relative to the largest score", np.abs(sf[f * N:(f + 1) * N] - sr).max() / sr.max(),
           2e-7, stated=1e-4)
    # the frame on its own (another buffer, another alignment): the same images bit for bit
    eng.set_frame(frames[f]["xyz"], None, h, w, cam)
    one = np.zeros((N, Pm), np.float32)
    eng.reproject(ph[f * N:(f + 1) * N], err=one)
    assert np.array_equal(one, got)


# ---- 5. the census --------------------------------------------------------------------------------------------------------------------------
def test_range_census(eng, synth):
    fr = synth.chess_like_frame(H, W, seed=2305)
    eng.set_frame(fr["xyz"], None, H, W, fr["cam"])
    poses, _, _ = eng.sample(256, seed=4711, thr=10.0, max_tries=1 << 16)
    assert np.abs(fr["xyz"]).max() < 6.0e4
    assert eng.k2_census(poses) == (0, 0)
    # a band of far coordinates: row 100, every coordinate beyond 70 m, nothing else beyond 60 m
    xyz = fr["xyz"].copy()
    band = slice(100 * W, 101 * W)
    xyz[band] = np.where(xyz[band] < 0, -1.0e5, 1.0e5).astype(np.float32) + xyz[band]
    assert np.abs(xyz[band]).min() > 7.0e4
    far = (np.abs(xyz) > 6.5e4).any(axis=1)
    chunks = np.add.reduceat(far.astype(np.int64), np.arange(0, P, 64)) > 0  # the kernel's chunking: 64 consecutive cells
    expect = int(chunks.sum())
    assert expect == 10
    eng.set_frame(xyz, None, H, W, fr["cam"])
    assert eng.k2_census(poses) == (expect, 0)
    # a translation beyond the records' range and a pose that is not a number
    bad = poses.copy()
    bad[7, 5] = 2.0e5
    bad[100] = np.nan
    assert eng.k2_census(bad) == (expect, 2)
    # a frame batch counts every frame's chunks
    import torch
    both = torch.from_numpy(np.ascontiguousarray(np.stack([xyz, fr["xyz"], xyz]))).cuda()
    eng.set_frames(both, None, H, W, fr["cam"], borrow=True)
    assert eng.k2_census(bad) == (2 * expect, 2)
    # K2 itself is untouched by the census: it still reports the exact form on this frame
    eng.set_frame(xyz, None, H, W, fr["cam"])
    soft = np.zeros(256)
    eng.reproject(poses, soft=soft)
    assert eng.k2_form() == (VEC, 0)
