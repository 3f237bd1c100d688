#!/usr/bin/env python3
"""Same bits from two builds of the library, for refactors of the K2 stage (k2_plan.h, dk::reproject, k2_stage): the sibling of scripts/same_bits.py.  The six
entry points that launch K2 (the calls of tests/test_gpu_k2_stage.py, plus dsac_score_sampled without the cv poses) run at N = 128 on six frames under every
option set that selects another form, another kernel or a refusal.  Per call the return code, the error text (the quoted call expression of a HIP failure and
addresses left out), "k2_form_last" / "k2_form_why_last", the number of K2 launches the profiling hook counted and every output array are dumped -- once per
library, each in a fresh child process with DSAC_HIP_LIB pointing at that library -- and the two dumps are compared byte for byte.  Any difference fails, and
the old library's dump must show every K2 form and every reason bit.

    python scripts/k2_same_bits.py --old <parent's libdsac_hip.so> --new dsac_amd/libdsac_hip.so [--out profiles/k2_plan_same_bits.txt]
    python scripts/k2_same_bits.py --dump FILE.npz        (what the children run)"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 128
BIT = lambda *k: sum(1 << i for i in k)
# (name, k2_variant, k2_flags, k2_exact_auto)
OPTIONS = ([("defaults", -1, 0, 1), ("exact_auto 0", -1, 0, 0)] + [("bit %d" % b, -1, BIT(b), 1) for b in (25, 27, 28, 29, 24)] +
           [("variant %d" % v, v, 0, 1) for v in (0, 21, 42, 45, 58, 61)] + [("variant 81 + bit 27", 81, BIT(27), 1)] +
           [("variant %d + bit 28" % v, v, BIT(28), 1) for v in (84, 85, 89, 93, 94, 95)] + [("variant 42 + bit 29", 42, BIT(29), 1)])
# the 16-bit element types with both store layouts ("k2_f16_store"); the entry points that take them: dsac_reproject_*, dsac_process_images_begin_*
OPTIONS16 = [("%s, k2_f16_store %d" % (e, st), e, st) for e in ("f16", "bf16") for st in (0, 1)]


def scenes():
    """name -> the scene dicts of tests/test_gpu_k2_stage.py (frames on the device); err_off: floats the error images start behind a 16-byte address"""
    import torch
    from dsac_amd import synth
    dev = torch.device("cuda", 0)
    cam = synth.CAM_7SCENES
    out = {}
    for name, h, w, grid, F, focal, err_off in (("40x40 uv", 40, 40, False, 1, None, 0), ("53x37 grid", 37, 53, True, 1, None, 0), ("64x64 grid", 64, 64, True, 1, None, 0),
                                                ("40x40 uv, err 4 bytes off", 40, 40, False, 1, None, 1), ("40x40 uv, f 1100", 40, 40, False, 1, 1100.0, 0),
                                                ("2 x 40x40 uv", 40, 40, False, 2, None, 0)):
        c = cam if focal is None else (focal, focal, cam[2], cam[3])
        frs = [synth.chess_like_frame(h, w, seed=5 + f, grid_uv=grid, cam=c) for f in range(F)]
        xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frs]))
        uv = np.ascontiguousarray(np.stack([fr["uv"] for fr in frs]))
        out[name] = dict(name=name, H=h, W=w, P=h * w, F=F, NT=N * F, cam=frs[0]["cam"], perm=torch.from_numpy(synth.fast_permutations(h * w, 8)).to(dev),
                         xyz=torch.from_numpy(xyz if F > 1 else xyz[0]).to(dev), uv=None if grid else torch.from_numpy(uv if F > 1 else uv[0]).to(dev), err_off=err_off)
    torch.cuda.synchronize(dev)
    return out


def clean(msg):
    msg = re.sub(r"^dsac_hip error -?\d+: ", "", msg)
    msg = re.sub(r"^.* failed: ", "<call> failed: ", msg)  # HIP_TRY quotes the call expression
    return re.sub(r"0x[0-9a-f]{6,}", "<address>", msg)


def dump(path):
    import torch
    import dsac_amd
    from dsac_amd import capi
    import test_gpu_k2_stage as T
    dev = torch.device("cuda", 0)
    eng = dsac_amd.Engine(0)
    out, meta = {}, {}

    def options(variant, flags, auto, f16_store=1):
        for k, v in (("k2_variant", variant), ("k2_flags", flags), ("k2_exact_auto", auto), ("k2_f16_store", f16_store), ("pi_defer_tail", 0)):
            eng.set_option(k, v)

    def run(key, s, b, keys, call):
        """one call: what it returned, what the context reports, what it wrote"""
        eng.synchronize()
        eng.profile_read(0)
        eng.profile_enable(True)
        rc, msg = 0, ""
        try:
            call()
        except capi.DsacError as e:
            rc, msg = e.code, clean(str(e))
        T._finish(eng)
        form, why = eng.get_option("k2_form_last"), eng.get_option("k2_form_why_last")
        meta[key] = dict(rc=rc, error=msg, form=form, why=why, launches=eng.profile_read(0)[1])
        for k in keys:
            out["%s/%s" % (key, k)] = (b[k].view(torch.int16) if b[k].dtype in (torch.float16, torch.bfloat16) else b[k]).cpu().numpy()
        if rc != 0:  # a refused call may leave a slot sampled or a begin open
            T._restore(eng, s)
        return rc

    for sname, s in scenes().items():
        T._set(eng, s)
        options(-1, 0, 1)
        b0 = T._bufs(s)  # the default call's poses: what dsac_reproject scores when the option set's first call is refused
        T._fused(eng, s, b0, False)
        T._finish(eng)
        for oname, variant, flags, auto in OPTIONS:
            first = {}
            calls = list(T._entry_points(lambda: first.get("poses", b0["poses"])))
            calls.insert(3, ("score_sampled without poses", ("scores", "w"), T._ahead, lambda e, s_, b: e.scoreSampled(0, None, b["scores"], b["w"], ent=b["entropy"],
                             avg=None, err=b["err"], tau=T.TAU, beta=T.BETA, scale=T.SCALE)))
            for cname, keys, before, call in calls:
                b = T._bufs(s)
                if s["err_off"]:
                    flat = torch.zeros(s["NT"] * s["P"] + 4, dtype=torch.float32, device=dev)
                    b["err"] = flat[s["err_off"]:s["err_off"] + s["NT"] * s["P"]].view(s["NT"], s["P"])
                    torch.cuda.synchronize(dev)
                T._set(eng, s)
                options(variant, flags, auto)
                if before:
                    before(eng, s, b)
                rc = run("%s/%s/%s" % (sname, oname, cname), s, b, ("err",) + tuple(keys), lambda: call(eng, s, b))
                if rc == 0 and not first and "poses" in keys:
                    first.update(b)
        for oname, elem, store in OPTIONS16:
            dt = torch.float16 if elem == "f16" else torch.bfloat16
            for cname in ("reproject", "process_images_begin"):
                b = T._bufs(s)
                flat = torch.zeros(s["NT"] * s["P"] + 8, dtype=dt, device=dev)
                b["err"] = flat[2 * s["err_off"]:2 * s["err_off"] + s["NT"] * s["P"]].view(s["NT"], s["P"])
                torch.cuda.synchronize(dev)
                T._set(eng, s)
                options(-1, 0, 1, store)
                if cname == "reproject":
                    call = lambda: eng.reproject(b0["poses"], N=s["NT"], err=b["err"], soft=b["scores"], tau=T.TAU, beta=T.BETA)
                else:
                    call = lambda: T._begin(eng, s, b)
                run("%s/%s/%s" % (sname, oname, cname), s, b, ("err", "scores"), call)
        T._restore(eng, s)
    eng.close()
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    np.savez(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print("%d calls, %d arrays -> %s" % (len(meta), len(out) - 1, path), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--old")
    ap.add_argument("--new")
    ap.add_argument("--dir", default=None, help="where the two dumps go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k2_plan_same_bits.txt"))
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
        return 0
    where = a.dir or tempfile.mkdtemp()
    os.makedirs(where, exist_ok=True)
    files = []
    for tag, lib in (("old", a.old), ("new", a.new)):
        files.append(os.path.join(where, "k2_same_bits_%s.npz" % tag))
        env = dict(os.environ, DSAC_HIP_LIB=os.path.abspath(lib))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", files[-1]], env=env, check=True, timeout=420)  # a failed child ends the run
    A, B = np.load(files[0]), np.load(files[1])
    mA, mB = (json.loads(bytes(d["meta"]).decode()) for d in (A, B))
    from dsac_amd import capi
    lines = ["# scripts/k2_same_bits.py: the K2 entry points at N = 128, old library against new: return code, error text, form, reason, K2 launches counted and",
             "# every output array, compared byte for byte.  Per frame and option set: calls (refused), forms that ran, arrays, bytes",
             "# old: %s" % a.old, "# new: %s" % a.new]
    bad = [] if set(A.files) == set(B.files) and set(mA) == set(mB) else ["the two dumps hold different calls or arrays"]
    forms = sorted({m["form"] for m in mA.values() if m["rc"] == 0})
    whys = sorted({bit for m in mA.values() if m["rc"] == 0 for bit in (1, 2, 4, 8) if m["why"] & bit})
    lines.append("forms in the old dump: %s;  reason bits: %s;  refused calls: %d of %d" % (", ".join("%d %s" % (f, capi.K2_FORMS[f]) for f in forms), whys,
                                                                                         sum(m["rc"] != 0 for m in mA.values()), len(mA)))
    if forms != [1, 2, 3, 4, 5, 6] or whys != [1, 2, 4, 8]:
        bad.append("the old dump does not show every form and every reason bit")
    groups = {}
    for k in sorted(mA):
        g = groups.setdefault(tuple(k.split("/")[:2]), dict(calls=0, refused=0, forms=set(), arrays=0, bytes=0, differ=0))
        g["calls"] += 1
        g["refused"] += mA[k]["rc"] != 0
        if mA[k]["rc"] == 0:
            g["forms"].add(mA[k]["form"])
        if mA[k] != mB.get(k):
            g["differ"] += 1
            bad.append("%s: %s != %s" % (k, mA[k], mB.get(k)))
    for k in sorted(A.files):
        if k == "meta":
            continue
        x, y = A[k], B[k] if k in B.files else None
        same = y is not None and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        g = groups[tuple(k.split("/")[:2])]
        g["arrays"] += 1
        g["bytes"] += x.nbytes
        if not same:
            g["differ"] += 1
            bad.append(k)
    for (sname, oname), g in groups.items():
        lines.append("%-26s %-22s %2d calls (%d refused)  forms %-9s %3d arrays %9d bytes  %s" % (sname, oname, g["calls"], g["refused"], sorted(g["forms"]), g["arrays"], g["bytes"],
                                                                                                 "identical" if not g["differ"] else "%d DIFFER" % g["differ"]))
    lines.append("RESULT: %s" % ("identical, %d calls, %d arrays" % (len(mA), len(A.files) - 1) if not bad else "FAILED: %s" % bad[:12]))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
