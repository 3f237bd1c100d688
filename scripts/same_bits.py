#!/usr/bin/env python3
"""Same bits from two builds of the library: for refactors of the refinement loops (dsac_refine_soft, dsac_refine_soft_backward, dsac_refine_rgbd) and of the
guided-sampling state (the six sampling-weight calls, dsac_sample, dsac_sample_rgbd).  Every output array of a fixed list of small calls is dumped once per
library, each in a fresh child process with DSAC_HIP_LIB pointing at that library, and the two dumps are compared byte for byte.  Any difference fails.

    python scripts/same_bits.py --old <parent's libdsac_hip.so> --new dsac_amd/libdsac_hip.so [--out profiles/soft_loop_same_bits.txt]
    python scripts/same_bits.py --dump FILE.npz        (what the children run)

The shapes are the smallest that reach every branch of the shared code: one chunk with a partial trip (63 x 1), 33 chunks (129 x 64), a ragged last chunk
(401 x 164, RGB-D), frame batches with a shuffled frame_of and a frame without problems, a first VALID cell beyond cell 256, B = 1 and 70, max_iters 1 / 2 / 20,
step_tol 0 / 1e-6, cut 60 / 100, start poses that are non-finite, far, and on a ladder of displacements from 1/16 to 16 times (0.03 rad, 40 mm).  The old
library's dump must show every status in both loops."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATUS = ("CONVERGED", "MAXIT", "SCORE", "FEW", "SINGULAR", "NONFINITE")
LOOP_PARAMS = ((1, 1e-6), (2, 0.0), (20, 1e-6), (20, 0.0))  # max_iters, step_tol


def grid_cam(H, W):
    return (525.0 * W / 640, 525.0 * W / 640, W / 2.0, H / 2.0)


def start_poses(gt, B, rng, rot, trans):
    """B start poses around gt (B x 6, one ground truth per problem): a ladder of displacements, then a NaN entry, an infinite one, a far pose, the zero pose
    and the ground truth itself"""
    p = np.array(gt, np.float64).reshape(B, 6).copy()
    if B < 6:  # a single problem: a small displacement
        p += np.concatenate([rng.normal(scale=rot, size=3), rng.normal(scale=trans, size=3)])
        return p
    for b in range(B - 5):
        s = 2.0 ** (8.0 * b / (B - 6) - 4.0)
        p[b] += s * np.concatenate([rng.normal(scale=rot, size=3), rng.normal(scale=trans, size=3)])
    p[B - 5, 4] = np.nan
    p[B - 4, 0] = np.inf
    p[B - 3, 3:] += 5000.0
    p[B - 2] = 0.0
    return p


def dump_soft(eng, out):
    from dsac_amd import synth
    rng = np.random.default_rng(11)
    maps = []
    for name, H, W, seeds in (("63x1", 1, 63, (46,)), ("129x64", 64, 129, (47,)), ("3x40x40", 40, 40, (48, 49, 50))):
        fr = [synth.chess_like_frame(H, W, seed=s, cam=grid_cam(H, W), grid_uv=True) for s in seeds]
        maps.append((name, H, W, np.stack([f["xyz"] for f in fr]), np.stack([f["gt_pose"] for f in fr]), max(2.0, H * W / 32.0)))
    one = np.full((1, 15, 3), np.nan, np.float32)  # one finite cell on the optical axis: the zero pose meets a pivot of exactly zero
    one[0, 7] = (0.0, 0.0, 1000.0)
    maps.append(("one_live3x5", 3, 5, one, np.zeros((1, 6)), 0.5))
    for name, H, W, xyz, gt, min_soft in maps:
        F = xyz.shape[0]
        cam = (525.0, 525.0, 2.0, 1.0) if name == "one_live3x5" else grid_cam(H, W)
        if F == 1:
            eng.set_frame(xyz[0], None, H, W, cam)
            runs = [("B70", 70, None), ("B1", 1, None)]
        else:
            eng.set_frames(xyz, None, H, W, cam)
            fo = rng.permutation(np.repeat(np.int32([0, 2]), 35)).astype(np.int32)  # frame 1 has no problem
            runs = [("B70of", 70, fo), ("B69", 69, None)]
        for tag, B, fo in runs:
            of = fo if fo is not None else (np.arange(B) // (B // F)).astype(np.int32)
            poses = start_poses(gt[of], B, rng, 0.03, 40.0)
            if name == "one_live3x5":
                poses[0] = 0.0
            for form in (0, 1):
                eng.set_option("refine_soft_form", form)
                for max_iters, step_tol in LOOP_PARAMS:
                    r = eng.refineSoft(poses, frame_of=fo, tau=10.0, beta=0.5, cut=42.0, min_soft=min_soft, max_iters=max_iters, step_tol=step_tol)
                    key = "soft/%s/%s/form%d/it%d_tol%g" % (name, tag, form, max_iters, step_tol)
                    for k, v in zip(("poses", "S", "iters", "status"), r):
                        out["%s/%s" % (key, k)] = v
                    if form == 0 and (max_iters, step_tol) == (20, 1e-6):
                        ref = r[0]
            dL = rng.normal(size=(B, 6))
            for fixed in (False, True):
                g, ok = eng.dRefineSoft(ref, dL, frame_of=fo, tau=10.0, beta=0.5, cut=42.0, min_soft=min_soft, fixed_weights=fixed)
                out["soft_bwd/%s/%s/fixed%d/grad" % (name, tag, fixed)] = g
                out["soft_bwd/%s/%s/fixed%d/ok" % (name, tag, fixed)] = ok
    eng.set_option("refine_soft_form", -1)


def dump_rgbd(eng, out):
    from dsac_amd import synth
    rng = np.random.default_rng(12)
    maps = []
    for name, H, W, seeds in (("63x1", 1, 63, (56,)), ("129x64", 64, 129, (57,)), ("401x164", 164, 401, (58,)), ("3x40x40", 40, 40, (59, 60, 61))):
        fr = [synth.chess_like_frame_rgbd(H, W, seed=s, cam=grid_cam(H, W), grid_uv=True, missing_frac=0.1) for s in seeds]
        pts = np.stack([f["cam_xyz"] for f in fr])
        if len(seeds) > 1:
            pts[1, :300] = np.nan  # the first VALID cell of frame 1 lies beyond cell 256
        maps.append((name, H, W, np.stack([f["xyz"] for f in fr]), pts, np.stack([f["gt_pose"] for f in fr])))
    fr = synth.chess_like_frame_rgbd(40, 40, seed=62, cam=grid_cam(40, 40), grid_uv=True, missing_frac=0.0)
    one = np.full((1, 1600, 3), np.nan, np.float32)
    cell = int(np.flatnonzero(fr["inlier_mask"])[0])  # a single VALID cell, and one that agrees with the ground truth: S >= min_soft, and the step is singular
    one[0, cell] = fr["cam_xyz"][cell]
    maps.append(("one_valid40x40", 40, 40, fr["xyz"][None], one, fr["gt_pose"][None]))
    for name, H, W, xyz, pts, gt in maps:
        F = xyz.shape[0]
        if F == 1:
            eng.set_frame(xyz[0], None, H, W, grid_cam(H, W))
            runs = [("B27", 27, None), ("B1", 1, None)]
        else:
            eng.set_frames(xyz, None, H, W, grid_cam(H, W))
            fo = rng.permutation(np.repeat(np.int32([1, 2]), 15)).astype(np.int32)  # frame 0 has no problem
            runs = [("B30of", 30, fo), ("B27", 27, None)]
        eng.set_camera_points(pts)
        for tag, B, fo in runs:
            of = fo if fo is not None else (np.arange(B) // (B // F)).astype(np.int32)
            poses = start_poses(gt[of], B, rng, 0.02, 30.0)
            for min_soft, cut in ((0.1 if name == "one_valid40x40" else 50.0, 100.0), (5.0, 60.0)):
                for max_iters, step_tol in LOOP_PARAMS:
                    r = eng.refineRGBD(poses, frame_of=fo, tau=100.0, beta=0.05, cut=cut, min_soft=min_soft, max_iters=max_iters, step_tol=step_tol)
                    key = "rgbd/%s/%s/soft%g_cut%g/it%d_tol%g" % (name, tag, min_soft, cut, max_iters, step_tol)
                    for k, v in zip(("poses", "S", "iters", "status"), r):
                        out["%s/%s" % (key, k)] = v


def dump_guided(eng, out):
    from dsac_amd import synth
    rng = np.random.default_rng(13)
    N = 64
    for H, W in ((40, 40), (64, 129)):
        P = H * W
        cam = grid_cam(H, W)
        fr = [synth.chess_like_frame_rgbd(H, W, seed=70 + f, cam=cam, grid_uv=True, missing_frac=0.1) for f in range(3)]
        for F in (1, 3):
            xyz, pts = np.stack([f["xyz"] for f in fr[:F]]), np.stack([f["cam_xyz"] for f in fr[:F]])
            n = F * N

            def set_frames():
                if F == 1:
                    eng.set_frame(xyz[0], None, H, W, cam)
                else:
                    eng.set_frames(xyz, None, H, W, cam)

            def options():
                return eng.get_option("sampling_weights"), eng.get_option("sampling_weights_rgbd")

            draw2 = lambda: eng.sample(n, seed=9, thr=10.0, max_tries=4096)
            draw3 = lambda: eng.sampleRGBD(n, seed=9, thr=100.0, max_tries=4096)
            set_frames()
            eng.set_camera_points(pts)
            uni2, uni3 = draw2(), draw3()
            g = rng.normal(size=n)
            for wname, w in (("ones", np.ones((F, P), np.float32)), ("half", (rng.random((F, P)) < 0.5).astype(np.float32))):
                key = "guided/%dx%d/F%d/%s" % (W, H, F, wname)
                # RGB-D first: dsac_sample_rgbd refuses while the 2D weights are active
                eng.set_sampling_weights_rgbd(w)
                assert options() == (0, 1)
                out[key + "/rgbd/table"] = eng.sampling_table_rgbd()
                r = draw3()
                for k, v in zip(("poses", "sets", "ok"), r):
                    out["%s/rgbd/%s" % (key, k)] = v
                out[key + "/rgbd/grad"] = eng.sampling_weights_backward_rgbd(r[1], r[2], g)
                eng.set_sampling_weights(w)
                assert options() == (1, 1)
                out[key + "/2d/table"] = eng.sampling_table()
                r = draw2()
                for k, v in zip(("poses", "sets", "ok"), r):
                    out["%s/2d/%s" % (key, k)] = v
                out[key + "/2d/grad"] = eng.sampling_weights_backward(r[1], r[2], g)
                # new camera points clear the RGB-D weights and nothing else; a set-frame call clears both kinds and the points
                eng.set_sampling_weights(None)
                eng.set_camera_points(pts)
                assert options() == (0, 0)
                r = draw3()
                assert all(np.array_equal(a, b) for a, b in zip(r, uni3)), key
                eng.set_sampling_weights(w)
                eng.set_sampling_weights_rgbd(w)
                assert options() == (1, 1)
                set_frames()
                assert options() == (0, 0)
                r = draw2()
                assert all(np.array_equal(a, b) for a, b in zip(r, uni2)), key
                eng.set_camera_points(pts)
                assert options() == (0, 0)
                r = draw3()
                assert all(np.array_equal(a, b) for a, b in zip(r, uni3)), key
            for k, v in zip(("poses", "sets", "ok"), uni2):
                out["guided/%dx%d/F%d/uniform/2d/%s" % (W, H, F, k)] = v
            for k, v in zip(("poses", "sets", "ok"), uni3):
                out["guided/%dx%d/F%d/uniform/rgbd/%s" % (W, H, F, k)] = v


def dump(path):
    import dsac_amd
    out = {}
    eng = dsac_amd.Engine(0)
    dump_soft(eng, out)
    dump_rgbd(eng, out)
    dump_guided(eng, out)
    eng.close()
    np.savez(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print("%d arrays -> %s" % (len(out), path), flush=True)


def statuses(d, prefix):
    seen = np.zeros(6, np.int64)
    for k in d.files:
        if k.startswith(prefix) and k.endswith("/status"):
            seen += np.bincount(d[k], minlength=6)[:6]
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--old")
    ap.add_argument("--new")
    ap.add_argument("--dir", default=None, help="where the two dumps go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_loop_same_bits.txt"))
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
        return 0
    where = a.dir or tempfile.mkdtemp()
    os.makedirs(where, exist_ok=True)
    files = []
    for tag, lib in (("old", a.old), ("new", a.new)):
        files.append(os.path.join(where, "same_bits_%s.npz" % tag))
        env = dict(os.environ, DSAC_HIP_LIB=os.path.abspath(lib))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", files[-1]], env=env, check=True, timeout=280)  # a failed child ends the run
    A, B = np.load(files[0]), np.load(files[1])
    lines = ["# scripts/same_bits.py: every output array of the listed calls, old library against new, compared byte for byte",
             "# old: %s" % a.old, "# new: %s" % a.new]
    bad = [] if set(A.files) == set(B.files) else ["the two dumps hold different arrays"]
    for prefix in ("soft/", "rgbd/"):
        seen = statuses(A, prefix)
        lines.append("statuses in the old dump, %-5s %s" % (prefix, "  ".join("%s %d" % (s, n) for s, n in zip(STATUS, seen))))
        if not (seen > 0).all():
            bad.append("%s: the old dump does not show every status" % prefix)
    groups = {}
    for k in sorted(A.files):
        x, y = A[k], B[k] if k in B.files else None
        same = y is not None and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        g = groups.setdefault("/".join(k.split("/")[:2]), [0, 0, 0])
        g[0] += 1
        g[1] += x.nbytes
        g[2] += 0 if same else 1
        if not same:
            bad.append(k)
    for name, (n, nbytes, diff) in groups.items():
        lines.append("%-28s %4d arrays %10d bytes  %s" % (name, n, nbytes, "identical" if not diff else "%d DIFFER" % diff))
    lines.append("RESULT: %s" % ("identical, %d arrays" % len(A.files) if not bad else "FAILED: %s" % bad[:12]))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
