"""The pipelined pair (dsac_sample_ahead / dsac_score_sampled) over frames that differ in MORE than their coordinates: intrinsics, map geometry, pixel
positions (sampled / implicit grid) and frame count change from one step to the next.  A slot is scored against the frame it was sampled from, and that
frame is all of it: the exact-transform K2 (the default) and the two-piece records (k2_flags bit 27) fold fx, fy and the split exponent into records that are
built right in front of the launch -- from the slot's frame, not from the one that is current at score time.  Every step is checked
  * against the fused call (dsac_score_hypotheses / dsac_score_hypotheses_frames) on that frame alone, bit for bit, error images included,
  * through dsac_get_option "k2_form_last" / "k2_form_why_last": the form that ran is the one this frame's focal length and geometry call for,
  * against the CPU oracle on the kernel's own poses: residuals, soft-inlier scores, softmax and soft-argmax pose at the tolerances of SURVEY.md 8(c).
The loop is the steady-state one: set the next frame, sample it ahead, score the current slot, no synchronisation until the end (one error-image buffer per
step).  The references (fused calls, oracle images) are computed once per module and shared."""
import numpy as np
import pytest

from conftest import excl_clamp_edge, margin

pytestmark = pytest.mark.gpu

# every step but the last is followed by a frame of another focal length; step 2 is followed by f > 2^10 (no split records), step 3 is itself f > 2^10
CAMS = ((525.0, 525.0, 320.0, 240.0), (585.0, 585.0, 320.0, 240.0), (700.3, 651.7, 301.5, 255.25), (1100.0, 1100.0, 320.0, 240.0),
        (262.5, 262.5, 160.0, 120.0), (1024.0, 1024.0, 320.0, 240.0), (525.0, 525.0, 320.0, 240.0))
FOCAL_STEP = 3  # the f = 1100 frame: the auto policy's fp32 form, DSAC_K2_WHY_FOCAL
H, W, N = 120, 160, 128
TAU, BETA, SCALE, CLAMP = 10.0, 0.5, 0.1, 100.0
EXACT_ANY, RECLO, PRECISE = 1 << 29, 1 << 27, 1 << 25
VEC, ANY = "exact (vector build)", "exact (any-map build)"
KEYS = ("poses", "sets", "ok", "scores", "w", "entropy", "avg")


def _defaults(engine):
    engine.set_option("k2_variant", -1)
    engine.set_option("k2_flags", 0)
    engine.set_option("k2_exact_auto", 1)


def _restore(engine):
    """What every test leaves behind, passed or failed: the default K2 options, and no slot sampled but not scored (the engine is the session's: a loop that
    stopped half way would otherwise fail every later dsac_sample_ahead on that slot)."""
    import torch
    from dsac_amd import capi
    engine.synchronize()
    _defaults(engine)
    dev = torch.device("cuda", 0)
    scores, w = torch.zeros(2 * N, dtype=torch.float64, device=dev), torch.zeros(2 * N, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    for k in (0, 1):
        try:
            engine.scoreSampled(k, None, scores, w)
        except capi.DsacError:
            pass  # nothing pending on this slot: the normal case
    engine.synchronize()


def _step(synth, h, w, frame_seed, sample_seed, cam, grid=False, nframes=1):
    """One step of a loop: `nframes` frames of h x w on the device (borrowed by the engine, so they stay referenced here until the module is done)."""
    import torch
    dev = torch.device("cuda", 0)
    frs = [synth.chess_like_frame(h, w, seed=frame_seed + f, cam=cam, grid_uv=grid) for f in range(nframes)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frs]))
    uv = np.ascontiguousarray(np.stack([fr["uv"] for fr in frs]))  # a batch carries one table of sampled positions per frame
    return dict(H=h, W=w, P=h * w, cam=tuple(float(c) for c in cam), F=nframes, N=N * nframes, seed=sample_seed, xyz=xyz, uv=uv,
                xyz_d=torch.from_numpy(xyz if nframes > 1 else xyz[0]).to(dev),
                uv_d=None if grid else torch.from_numpy(uv if nframes > 1 else uv[0]).to(dev))


def _set(engine, s):
    if s["F"] > 1:
        engine.set_frames(s["xyz_d"], s["uv_d"], s["H"], s["W"], s["cam"], uv_per_frame=s["uv_d"] is not None, borrow=True)
    else:
        engine.set_frame(s["xyz_d"], s["uv_d"], s["H"], s["W"], s["cam"], borrow=True)


def _reference(engine, orc, s):
    """The fused call on this step's frame(s) alone under the default options, the range census of its poses, and the oracle's images of those poses."""
    _set(engine, s)
    err = np.zeros((s["N"], s["P"]), np.float32)
    if s["F"] > 1:
        out = engine.scoreHypothesesFrames(N, seed=s["seed"], scale=SCALE, err=err)
    else:
        out = engine.scoreHypotheses(s["N"], seed=s["seed"], scale=SCALE, err=err)
    s["fused"] = dict(zip(KEYS, out))
    s["fused"]["err"] = err
    s["fused_form"] = engine.k2_form()
    s["census"] = engine.k2_census(out[0])
    poses = out[0]
    s["orc_err"] = np.concatenate([orc.get_diff_maps(poses[f * N:(f + 1) * N], s["xyz"][f], s["uv"][f], s["H"], s["W"], s["cam"]) for f in range(s["F"])])
    s["orc_soft"] = np.concatenate([orc.soft_inlier(s["orc_err"][f * N:(f + 1) * N], TAU, BETA) for f in range(s["F"])])
    return s


@pytest.fixture(scope="module")
def cams(engine, orc, synth):
    """(a), (c), (d): seven 120 x 160 frames with sampled pixel positions, one camera each."""
    _defaults(engine)
    steps = [_reference(engine, orc, _step(synth, H, W, 900 + i, 40 + i, cam)) for i, cam in enumerate(CAMS)]
    engine.synchronize()
    yield steps
    engine.synchronize()


@pytest.fixture(scope="module")
def maps(engine, orc, synth):
    """(b): map geometry, pixel positions and frame count alternate.  37 x 53 has an odd cell count: the any-map build."""
    _defaults(engine)
    spec = (dict(h=120, w=160, cam=CAMS[0]), dict(h=96, w=128, cam=(117.0, 117.0, 64.0, 48.0), grid=True),
            dict(h=37, w=53, cam=(525.0 * 53 / 640, 525.0 * 53 / 640, 26.5, 18.5), grid=True), dict(h=120, w=160, cam=CAMS[0], nframes=2),
            dict(h=60, w=80, cam=CAMS[2]))
    # frame seed 930 + i (the batch: 933 and 934), sampling seed 60 + i.  On the CPU oracle the 128 poses of every step have |t| <= 9.8 m (the 37 x 53 step: 9.0 m)
    # against the 131 m the split records reach, and 0.69, 0.84, 0.95, 0.70 and 0.70 of the cells are off the clamp
    steps = [_reference(engine, orc, _step(synth, sp.pop("h"), sp.pop("w"), 930 + i, 60 + i, sp.pop("cam"), **sp)) for i, sp in enumerate(spec)]
    engine.synchronize()
    yield steps
    engine.synchronize()


def _run_pair(engine, steps, with_poses=True, score_last=True):
    """sample ahead / score over `steps` without a synchronisation; returns the per-step device buffers and the (form, why) read after each score call.
    score_last = False leaves the last slot sampled and pending."""
    import torch
    dev = torch.device("cuda", 0)
    z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
    bufs = [dict(poses=z(s["N"], 6), sets=z(s["N"], 4, dtype=torch.int32), ok=z(s["N"], dtype=torch.uint8), scores=z(s["N"]), w=z(s["N"]),
                 entropy=z(s["F"]), avg=z(s["F"], 6), err=z(s["N"], s["P"], dtype=torch.float32)) for s in steps]
    torch.cuda.synchronize(dev)  # the fills ran on torch's stream, the engine has its own
    forms = []
    S = len(steps)
    _set(engine, steps[0])
    engine.sampleAhead(0, steps[0]["N"], steps[0]["seed"], bufs[0]["poses"], bufs[0]["sets"], bufs[0]["ok"])
    for i in range(S):
        k = i & 1
        if i + 1 < S:
            _set(engine, steps[i + 1])  # the frame of the NEXT step becomes current ...
            nb = bufs[i + 1]
            engine.sampleAhead(1 - k, steps[i + 1]["N"], steps[i + 1]["seed"], nb["poses"], nb["sets"], nb["ok"])
        if i + 1 == S and not score_last:
            break
        b = bufs[i]
        engine.scoreSampled(k, b["poses"] if with_poses else None, b["scores"], b["w"], ent=b["entropy"], avg=b["avg"] if with_poses else None, err=b["err"],
                            scale=SCALE)  # ... while this one scores the frame of step i
        forms.append(engine.k2_form())  # host state
    return bufs, forms


def _host(b):
    return {k: v.cpu().numpy() for k, v in b.items()}


def _same_bits(tag, got, s, keys=KEYS + ("err",)):
    for key in keys:
        ref = s["fused"][key]
        assert np.array_equal(got[key].reshape(ref.shape), ref), "%s: %s differs from the fused call on this frame alone" % (tag, key)


def _residuals(tag, err, s, poses, tol, fp32=False):
    """error images against the oracle's on the same poses.  Exact forms: `tol` px on every cell off the clamp edge.  The fp32 form (the rule of
    test_random_shape): 1e-3 px at scene depth, |Ez| >= 200 mm, scaled by (Ez / 200)^2 nearer to the camera centre, where E = R X + t cancels."""
    ref = s["orc_err"]
    m = excl_clamp_edge(err, ref, CLAMP)
    d = np.abs(err - ref)
    # a condition, not a measurement: the oracle alone has 0.64-0.72 of the cells of (a)'s frames off the clamp (0.69-0.95 of (b)'s); a kernel that clamped
    # its way out of the comparison would show here
    assert m.mean() >= 0.6, "%s: only %.3f of the cells are off the clamp" % (tag, m.mean())
    assert (ref[err == np.float32(CLAMP)] >= CLAMP - 1e-3).all(), "%s: a cell was clamped that the oracle keeps below the clamp" % tag
    if not fp32:
        margin("a3", "pipelined pair, %s: K2 residuals vs oracle on the kernel's own poses, max px (clamp-edge cells excluded)" % tag, d[m].max(initial=0.0), tol)
        return
    from dsac_amd.synth import rodrigues
    Ez = np.concatenate([np.stack([(rodrigues(h6[:3])[2] * s["xyz"][f].astype(np.float64)).sum(1) + h6[5] for h6 in poses[f * N:(f + 1) * N]])
                         for f in range(s["F"])])
    scene = np.abs(Ez) >= 200.0
    margin("a3", "pipelined pair, %s: fp32 K2 residuals vs oracle, cells at scene depth (|Ez| >= 200 mm), max px (clamp-edge cells excluded)" % tag,
           d[m & scene].max(initial=0.0), tol)
    near = m & ~scene
    if near.any():
        margin("a3", "pipelined pair, %s: fp32 K2 residuals vs oracle, cells within 200 mm of the camera centre: max of |d| * (Ez / 200)^2 px" % tag,
               (d[near] * (Ez[near] / 200.0) ** 2).max(), tol)


def _scores_and_tail(tag, got, s, orc):
    margin("north*", "pipelined pair, %s: soft-inlier scores vs oracle, relative to the largest score" % tag,
           np.abs(got["scores"] - s["orc_soft"]).max() / max(1.0, np.abs(s["orc_soft"]).max()), 1e-4)
    for f in range(s["F"]):
        sl = slice(f * N, (f + 1) * N)
        margin("a4", "pipelined pair, %s: K3 softmax on the kernel's own scores vs oracle" % tag, np.abs(orc.softMax(SCALE * got["scores"][sl]) - got["w"][sl]).max(), 1e-12)
        margin("a5", "pipelined pair, %s: soft-argmax pose vs oracle on the same weights and poses" % tag,
               np.abs(orc.avg_pose(got["w"][sl], got["poses"][sl]) - got["avg"][f]).max(), 1e-9)


def _check_default_step(tag, i, got, form, s, orc, capi, focal):
    """What (a) asserts per step under the auto policy (and under bit 29 on the frames that take the exact form)."""
    _same_bits("%s step %d" % (tag, i), got, s)
    if focal:
        assert form[0].startswith("fp32") and form[1] == capi.DSAC_K2_WHY_FOCAL, (i, form)
    else:
        assert s["census"] == (0, 0), "step %d: precondition -- a hypothesis or a coordinate outside the split's range: %r" % (i, s["census"])
        assert form == (VEC, 0), (i, form)
    _residuals("%s%s" % (tag, ", f > 2^10" if focal else ""), got["err"], s, got["poses"], 1e-3, fp32=focal)
    _scores_and_tail(tag, got, s, orc)


def _each_slot_default(engine, orc, cams, tag):
    from dsac_amd import capi
    _defaults(engine)
    bufs, forms = _run_pair(engine, cams)
    engine.synchronize()
    assert len(forms) == len(cams)
    for i, s in enumerate(cams):
        _check_default_step(tag, i, _host(bufs[i]), forms[i], s, orc, capi, focal=i == FOCAL_STEP)


@pytest.mark.parametrize("flags", [0, EXACT_ANY, RECLO, PRECISE])
def test_each_slot_scores_with_its_own_intrinsics(engine, orc, cams, flags):
    """Seven frames, seven cameras: each step's K2 runs with records folded with ITS frame's fx, fy and split exponent, although the next frame is current
    when it is enqueued.  flags 0: the auto policy (exact form, fp32 for the f = 1100 frame).  Bit 29 (the exact form or an error): every frame up to the
    f = 1100 one succeeds -- also the one that is FOLLOWED by it --, the f = 1100 slot is refused, stays pending and scores once the flag is gone.  Bits 27 / 25
    (two-piece records / precise), without the f = 1100 frame: the error images of engine.reproject with the same flag on that frame alone."""
    from dsac_amd import capi
    try:
        if flags == 0:
            _each_slot_default(engine, orc, cams, "auto policy")
        elif flags == EXACT_ANY:
            _defaults(engine)
            engine.set_option("k2_flags", EXACT_ANY)
            steps = cams[:FOCAL_STEP + 1]
            bufs, forms = _run_pair(engine, steps, score_last=False)
            assert len(forms) == FOCAL_STEP
            b, k = bufs[FOCAL_STEP], FOCAL_STEP & 1
            with pytest.raises(capi.DsacError):
                engine.scoreSampled(k, b["poses"], b["scores"], b["w"], ent=b["entropy"], avg=b["avg"], err=b["err"], scale=SCALE)
            engine.synchronize()
            for i in range(FOCAL_STEP):
                _check_default_step("k2_flags bit 29", i, _host(bufs[i]), forms[i], steps[i], orc, capi, focal=False)
            # the rejected call left the slot sampled and pending: without the flag the same slot scores, in the fp32 form
            engine.set_option("k2_flags", 0)
            engine.scoreSampled(k, b["poses"], b["scores"], b["w"], ent=b["entropy"], avg=b["avg"], err=b["err"], scale=SCALE)
            form = engine.k2_form()
            engine.synchronize()
            _check_default_step("k2_flags bit 29, then 0", FOCAL_STEP, _host(b), form, steps[FOCAL_STEP], orc, capi, focal=True)
        else:
            name, tol = ("records in two pieces", 6e-3) if flags == RECLO else ("precise", 1e-3)  # 6e-3: what test_records_in_two_pieces asserts for that form
            _defaults(engine)
            engine.set_option("k2_flags", flags)
            steps = [s for i, s in enumerate(cams) if i != FOCAL_STEP]
            bufs, forms = _run_pair(engine, steps)
            engine.synchronize()
            for i, s in enumerate(steps):
                got = _host(bufs[i])
                _same_bits("k2_flags %#x step %d" % (flags, i), got, s, keys=("poses", "sets", "ok"))  # K1 knows no K2 flag
                assert forms[i] == (name, capi.DSAC_K2_WHY_FORCED), (i, forms[i])
                _set(engine, s)
                alone = np.zeros((s["N"], s["P"]), np.float32)
                engine.reproject(got["poses"], err=alone, tau=TAU, beta=BETA)
                assert engine.k2_form() == (name, capi.DSAC_K2_WHY_FORCED)
                assert np.array_equal(got["err"], alone), "step %d: error images differ from dsac_reproject with the same flag on this frame alone" % i
                _residuals(name, got["err"], s, got["poses"], tol)
    finally:
        _restore(engine)


def test_each_slot_scores_on_its_own_map(engine, orc, maps):
    """Map size, sampled / implicit pixel positions, vector / any-map build and one frame / a batch of two alternate from step to step: tiles, strides, the
    frame count and the build of the exact form are the slot's frame's."""
    try:
        _defaults(engine)
        bufs, forms = _run_pair(engine, maps)
        engine.synchronize()
        for i, s in enumerate(maps):
            tag = "%d x %dx%d%s" % (s["F"], s["H"], s["W"], " grid" if s["uv_d"] is None else "")
            got = _host(bufs[i])
            _same_bits("maps step %d (%s)" % (i, tag), got, s)
            assert s["census"] == (0, 0), "step %d: precondition -- a hypothesis or a coordinate outside the split's range: %r" % (i, s["census"])
            assert forms[i] == (ANY if s["P"] % 4 else VEC, 0) and forms[i] == s["fused_form"], (i, forms[i])
            _residuals("maps " + tag, got["err"], s, got["poses"], 1e-3)
            _scores_and_tail("maps " + tag, got, s, orc)
        assert [f[0] for f in forms].count(ANY) == 1
    finally:
        _restore(engine)


def test_scoring_without_poses_uses_the_slots_own_records(engine, orc, cams):
    """dsac_score_sampled without the cv poses has nothing to split: the fp32 form on the records K1 staged for the slot -- with the slot's focal lengths in
    them.  The same error images as the loop with poses and the exact form switched off ("k2_exact_auto" 0)."""
    from dsac_amd import capi
    steps = cams[:3]
    try:
        _defaults(engine)
        bufs, forms = _run_pair(engine, steps, with_poses=False)
        engine.synchronize()
        engine.set_option("k2_exact_auto", 0)
        bufs32, forms32 = _run_pair(engine, steps)
        engine.synchronize()
        for i, s in enumerate(steps):
            got, got32 = _host(bufs[i]), _host(bufs32[i])
            assert forms[i][0].startswith("fp32") and forms[i][1] & capi.DSAC_K2_WHY_NO_POSES, (i, forms[i])
            assert forms32[i][0] == forms[i][0] and forms32[i][1] == capi.DSAC_K2_WHY_AUTO_OFF, (i, forms32[i])
            _same_bits("no poses, step %d" % i, got, s, keys=("poses", "sets", "ok"))
            assert np.array_equal(got["err"], got32["err"]), "step %d: error images differ from the fp32 form with poses" % i
            assert np.array_equal(got["scores"], got32["scores"]) and np.array_equal(got["w"], got32["w"])
            _residuals("scored without poses", got["err"], s, got["poses"], 1e-3, fp32=True)
    finally:
        _restore(engine)


def test_each_slot_scores_with_its_own_intrinsics_while_profiling(engine, orc, cams):
    """dsac_profile_enable attaches an event pair to every K2 dispatch: the options of that launch (records, form) must still be the slot's frame's, the bits
    the same, and dsac_profile_read returns one launch per step."""
    try:
        engine.synchronize()
        engine.profile_read(0)  # drop what earlier launches left
        engine.profile_enable(True)
        _each_slot_default(engine, orc, cams, "auto policy, profiling")
        ms, launches = engine.profile_read(0)
        assert launches == len(cams) and ms > 0.0, (ms, launches)
    finally:
        engine.profile_enable(False)
        engine.profile_read(0)
        _restore(engine)
