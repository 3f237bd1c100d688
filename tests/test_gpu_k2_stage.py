"""Every K2 launch of the C ABI is assembled in one place (k2_stage in csrc/api.hip); six entry points reach it:
  dsac_score_hypotheses / _frames, in stream order and with the score tail deferred ("pi_defer_tail" 2 with device arrays),
  dsac_sample_ahead + dsac_score_sampled, dsac_process_images ("pi_defer_tail" 0 and 2), dsac_process_images_begin, dsac_reproject.
(a) On the same frame, seed and options they compute the same bits -- error images, scores / soft sums, softmax weights -- in the same arithmetic form, whatever
    records that form needs (split records, low parts, the cv poses themselves) and with or without a profiling pair attached to the launch.
(b) The dsac_set_k2_events gate surrounds five of them and not dsac_score_sampled.
(c) A launch that is refused leaves no trace: no profiling sample, no record of the gate's event, and the next call works.
Nothing here is compared against a tolerance: the entry points run the same kernels on the same records, so the comparison is bitwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128  # hypotheses per frame: the smallest count a frame batch allows
SEED = 4711
TAU, BETA, SCALE, CLAMP = 10.0, 0.5, 0.1, 100.0
EXACT_ANY, RECLO, PRECISE = 1 << 29, 1 << 27, 1 << 25
VEC, ANY = "exact (vector build)", "exact (any-map build)"
SHAPES = {"40x40": (40, 40), "53x37": (37, 53)}  # 1600 cells with sampled positions: the vector build; 1961 cells (odd) on the implicit grid: the any-map build
MODES = ("default", "reclo", "precise", "auto_off", "profiling")


def _defaults(engine):
    engine.set_option("k2_variant", -1)
    engine.set_option("k2_flags", 0)
    engine.set_option("k2_exact_auto", 1)
    engine.set_option("pi_defer_tail", 0)


def _set(engine, s):
    if s["F"] > 1:
        engine.set_frames(s["xyz"], s["uv"], s["H"], s["W"], s["cam"], uv_per_frame=s["uv"] is not None, borrow=True)
    else:
        engine.set_frame(s["xyz"], s["uv"], s["H"], s["W"], s["cam"], borrow=True)


def _restore(engine, s):
    """What every test leaves behind, passed or failed: default options, no gate, no profiling, no slot sampled but not scored, no begin without its finish."""
    from dsac_amd import capi
    engine.synchronize()
    _defaults(engine)
    engine.set_k2_events(None, None)
    engine.profile_enable(False)
    engine.profile_read(0)
    b = _bufs(s)
    for k in (0, 1):
        try:
            engine.scoreSampled(k, None, b["scores"], b["w"])
        except capi.DsacError:
            pass  # nothing pending on this slot: the normal case
    _set(engine, s)
    engine.processImages(N, s["perm"], seed=SEED, out=_pi_out(b))  # a whole call closes a begin that was left open
    engine.synchronize()


@pytest.fixture(scope="module")
def scenes(synth):
    """(shape, frames) -> the frame(s) on the device, borrowed by the engine (so they stay referenced here), and the refinement permutations."""
    import torch
    dev = torch.device("cuda", 0)
    out = {}
    for name, (h, w) in SHAPES.items():
        grid = name == "53x37"
        frs = [synth.chess_like_frame(h, w, seed=5 + f, grid_uv=grid) for f in range(2)]
        perm = torch.from_numpy(synth.fast_permutations(h * w, 8)).to(dev)
        for F in (1, 2):
            xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frs[:F]]))
            uv = np.ascontiguousarray(np.stack([fr["uv"] for fr in frs[:F]]))
            out[name, F] = dict(name=name, H=h, W=w, P=h * w, F=F, NT=N * F, cam=frs[0]["cam"], perm=perm,
                                xyz=torch.from_numpy(xyz if F > 1 else xyz[0]).to(dev), uv=None if grid else torch.from_numpy(uv if F > 1 else uv[0]).to(dev))
    torch.cuda.synchronize(dev)
    return out


def _bufs(s):
    """Fresh device arrays for one call (zero-filled on torch's stream: synchronised before the engine's own streams write them)."""
    import torch
    dev = torch.device("cuda", 0)
    z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
    NT, F = s["NT"], s["F"]
    b = dict(poses=z(NT, 6), sets=z(NT, 4, dtype=torch.int32), ok=z(NT, dtype=torch.uint8), scores=z(NT), w=z(NT), entropy=z(F), avg=z(F, 6),
             err=z(NT, s["P"], dtype=torch.float32), ref=z(F, 6), steps=z(F, dtype=torch.int32))
    torch.cuda.synchronize(dev)
    return b


def _pi_out(b):
    return dict(hyps=b["poses"], sampledPoints=b["sets"], ok=b["ok"], scores=b["scores"], sfScores=b["w"], sfEntropy=b["entropy"], avgHyp=b["avg"],
                refAvgHyp=b["ref"], refSteps=b["steps"])


def _fused(engine, s, b, defer):
    engine.set_option("pi_defer_tail", 2 if defer else 0)
    out = (b["poses"], b["sets"], b["ok"], b["scores"], b["w"], b["entropy"], b["avg"])
    if s["F"] > 1:
        engine.scoreHypothesesFrames(N, seed=SEED, tau=TAU, beta=BETA, scale=SCALE, err=b["err"], out=out)
    else:
        engine.scoreHypotheses(N, seed=SEED, tau=TAU, beta=BETA, scale=SCALE, err=b["err"], out=out)


def _ahead(engine, s, b):
    engine.sampleAhead(0, s["NT"], SEED, b["poses"], b["sets"], b["ok"])


def _sampled(engine, s, b):
    engine.scoreSampled(0, b["poses"], b["scores"], b["w"], ent=b["entropy"], avg=b["avg"], err=b["err"], tau=TAU, beta=BETA, scale=SCALE)


def _process(engine, s, b, mode):
    engine.set_option("pi_defer_tail", mode)
    engine.processImages(N, s["perm"], seed=SEED, tau=TAU, beta=BETA, scale=SCALE, err=b["err"], out=_pi_out(b))


def _begin(engine, s, b):
    engine.processImagesBegin(N, b["err"], seed=SEED, tau=TAU, beta=BETA, soft=b["scores"], out=(b["poses"], b["sets"], b["ok"]))


def _entry_points(first_poses):
    """(name, what the call leaves besides the error images, a step that runs before the call is counted, the call).  dsac_reproject runs on the poses of the
    first call, through `first_poses()`."""
    def reproject(engine, s, b):
        engine.reproject(first_poses(), N=s["NT"], err=b["err"], soft=b["scores"], tau=TAU, beta=BETA)
    return (("score_hypotheses", ("poses", "scores", "w"), None, lambda e, s, b: _fused(e, s, b, False)),
            ("score_hypotheses, tail deferred", ("poses", "scores", "w"), None, lambda e, s, b: _fused(e, s, b, True)),
            ("sample_ahead + score_sampled", ("poses", "scores", "w"), _ahead, _sampled),
            ("process_images", ("poses", "scores", "w"), None, lambda e, s, b: _process(e, s, b, 0)),
            ("process_images, tails deferred", ("poses", "scores", "w"), None, lambda e, s, b: _process(e, s, b, 2)),
            ("process_images_begin", ("poses", "scores"), None, _begin),
            ("reproject", ("scores",), None, reproject))


def _finish(engine):
    engine.joinTail()
    engine.synchronize()
    engine.set_option("pi_defer_tail", 0)


@pytest.mark.parametrize("frames", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_six_entry_points_agree(engine, scenes, shape, frames, mode):
    from dsac_amd import capi
    s = scenes[shape, frames]
    flags = {"reclo": RECLO, "precise": PRECISE}.get(mode, 0)
    expect = {"default": (VEC if shape == "40x40" else ANY, 0), "profiling": (VEC if shape == "40x40" else ANY, 0),
              "reclo": ("records in two pieces", capi.DSAC_K2_WHY_FORCED), "precise": ("precise", capi.DSAC_K2_WHY_FORCED), "auto_off": None}[mode]
    refused = flags != 0 and shape == "53x37"  # bits 25 / 27 name kernels that read 16-byte vectors: an error on a map of 1961 cells, never another form
    try:
        _defaults(engine)
        _set(engine, s)
        default_poses = None
        if refused:  # the poses dsac_reproject is given, and the form the refused calls must leave in place: the default call's
            b0 = _bufs(s)
            _fused(engine, s, b0, False)
            engine.synchronize()
            default_poses = b0["poses"]
            assert engine.k2_form() == (ANY, 0)
        engine.set_option("k2_flags", flags)
        engine.set_option("k2_exact_auto", 0 if mode == "auto_off" else 1)
        if mode == "profiling":
            engine.synchronize()
            engine.profile_read(0)  # drop what earlier launches left
            engine.profile_enable(True)
        first = {}
        for name, keys, before, call in _entry_points(lambda: default_poses if refused else first["poses"]):
            b = _bufs(s)
            if before:
                before(engine, s, b)
            if refused:
                with pytest.raises(capi.DsacError):
                    call(engine, s, b)
                _finish(engine)
                assert engine.k2_form() == (ANY, 0), "%s: a refused launch changed the form report" % name
                continue
            call(engine, s, b)
            form = engine.k2_form()  # host state
            _finish(engine)
            if mode == "profiling":
                ms, launches = engine.profile_read(0)
                assert launches == 1 and ms > 0.0, "%s: %d K2 launches sampled for one call" % (name, launches)
            if not first:
                first.update(b, form=form)
                assert bool(b["ok"].any()) and float(b["err"].min()) < CLAMP, "precondition: K1 found poses and K2 wrote residuals below the clamp"
                if expect is not None:
                    assert form == expect, form
                else:
                    assert form[0].startswith("fp32") and form[1] == capi.DSAC_K2_WHY_AUTO_OFF, form
                continue
            assert form == first["form"], "%s ran as %r, score_hypotheses as %r" % (name, form, first["form"])
            for key in ("err",) + keys:
                assert np.array_equal(b[key].cpu().numpy(), first[key].cpu().numpy()), "%s: %s differs from score_hypotheses" % (name, key)
    finally:
        _restore(engine, s)


def _gate(engine):
    """A completed event to wait for, a timing event to record (recorded once already, so that it has a time before any marker), and the engine's stream."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.ExternalStream(int(engine.stream), device=dev)
    done, gate = torch.cuda.Event(), torch.cuda.Event(enable_timing=True)
    done.record(st)
    gate.record(st)
    st.synchronize()
    engine.set_k2_events(wait_before=done, record_after=gate)
    return st, gate


def _gate_moved(engine, st, gate, call):
    """ms from a marker recorded on the engine's stream right before `call` to the gate's event: > 0 when the call recorded it again."""
    import torch
    marker = torch.cuda.Event(enable_timing=True)
    marker.record(st)
    try:
        call()
    finally:
        _finish(engine)
    return marker.elapsed_time(gate)


def test_the_gate_surrounds_five_entry_points_and_not_score_sampled(engine, scenes):
    s = scenes["40x40", 1]
    try:
        _defaults(engine)
        _set(engine, s)
        b0 = _bufs(s)
        _fused(engine, s, b0, False)  # poses for dsac_reproject
        engine.synchronize()
        st, gate = _gate(engine)  # wait_before has completed: nothing blocks
        for name, _, before, call in _entry_points(lambda: b0["poses"]):
            b = _bufs(s)
            if before:
                before(engine, s, b)
            ms = _gate_moved(engine, st, gate, lambda: call(engine, s, b))
            print("gate: %-34s record_after - marker = %+.4f ms" % (name, ms))
            if call is _sampled:
                assert ms < 0.0, "dsac_score_sampled recorded the gate's event (%.4f ms after the marker)" % ms
                assert np.array_equal(b["err"].cpu().numpy(), b0["err"].cpu().numpy())
            else:
                assert ms > 0.0, "%s did not record the gate's event (%.4f ms)" % (name, ms)
    finally:
        _restore(engine, s)


def test_a_refused_launch_leaves_no_trace(engine, scenes):
    """k2_variant 42 names an fp32 form, bit 29 asks for the exact one or an error: dsac_reproject is refused before any K2 kernel is enqueued."""
    from dsac_amd import capi
    s = scenes["40x40", 1]
    try:
        _defaults(engine)
        _set(engine, s)
        b0 = _bufs(s)
        _fused(engine, s, b0, False)
        engine.synchronize()
        form = engine.k2_form()
        st, gate = _gate(engine)
        engine.profile_read(0)
        engine.profile_enable(True)
        engine.set_option("k2_flags", EXACT_ANY)
        engine.set_option("k2_variant", 42)
        b = _bufs(s)

        def refused():
            with pytest.raises(capi.DsacError):
                engine.reproject(b0["poses"], N=s["NT"], err=b["err"], soft=b["scores"], tau=TAU, beta=BETA)
        ms = _gate_moved(engine, st, gate, refused)
        assert ms < 0.0, "the refused call recorded the gate's event (%.4f ms after the marker)" % ms
        assert engine.profile_read(0)[1] == 0
        assert engine.k2_form() == form
        engine.set_option("k2_variant", -1)
        ms = _gate_moved(engine, st, gate, lambda: engine.reproject(b0["poses"], N=s["NT"], err=b["err"], soft=b["scores"], tau=TAU, beta=BETA))
        assert ms > 0.0
        t, launches = engine.profile_read(0)
        assert launches == 1 and t > 0.0
        assert np.array_equal(b["err"].cpu().numpy(), b0["err"].cpu().numpy()) and np.array_equal(b["scores"].cpu().numpy(), b0["scores"].cpu().numpy())
    finally:
        _restore(engine, s)
