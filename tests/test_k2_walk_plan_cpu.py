"""The hypothesis walk of dk::k2_plan (dsac_amd/csrc/k2_plan.h: K2Plan::hyp_walk, "k2_hyp_walk") on the host, no GPU: over the sweep of plan inputs of
tests/test_k2_plan_cpu.py, and over frame batches and hypothesis counts chosen for the walk, with the option at 0 (auto), 1, 2 and 4 --
  * the walk is 1 wherever the kernel has no full-tile path, and under the auto policy wherever the launch is not in the big regime;
  * no walk straddles a frame or the end of N, and a forced walk is the longest legal one up to what was asked for;
  * the grid's walks times the walk cover every hypothesis tile exactly once (the pixel tiles are the plan's `tiles`, which the option must not change);
  * every other field of the plan equals the plan with the option at 1;
  * two planted mistakes -- a walk allowed across a frame boundary, a grid not divided by the walk -- are noticed by these same checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import k2_plan_ref as ref
import test_k2_plan_cpu as base

HERE = os.path.dirname(os.path.abspath(__file__))
IN_FIELDS = base.IN_FIELDS + ("hyp_walk",)
OUT_FIELDS = tuple(ref.FIELDS) + ("hyp_walk", "walks")
EXACT_VEC = 7          # K2_FAM_EXACT_VEC
BIG_BYTES = 1.0e9      # K2_BIG_BYTES
MIN_WGS = 8 * 2048     # K2_WALK_MIN_GENERATIONS fills of K2_WAVE_SLOTS


@pytest.fixture(scope="module")
def k2w(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("k2w") / "libk2w.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "helpers", "k2_walk_plan_host.cpp")])
    lib = C.CDLL(out)
    assert lib.k2w_in_fields() == len(IN_FIELDS) and lib.k2w_out_fields() == len(OUT_FIELDS)
    return lib


def _extra():
    """what the base sweep has little of: exact-form launches on 64-wide grids and 640 x 480 with hypothesis counts and frame batches either side of every
    legality condition (three tiles, a ragged tile, Nf of 128 / 256 / 384) and either side of the auto policy's regime"""
    rows = []
    for P, W in ((512, 64), (576, 64), (16640, 64), (307200, 640), (1600, 40)):
        for N, frames, Nf in ((64, 1, 0), (128, 1, 0), (192, 1, 0), (200, 1, 0), (256, 1, 0), (384, 3, 128), (512, 2, 256), (768, 2, 384), (768, 3, 256), (1024, 4, 256),
                              (1024, 1, 0), (2048, 8, 256), (4096, 16, 256), (4096, 1, 0), (4032, 1, 0), (8192, 32, 256)):
            for es in ((1, 1), (1, 0), (0, 1)):
                for elem in (0, 1, 2):
                    for flags in (0, 1 << 28, 1 << 30):
                        rows.append(dict(flags=flags, exact_auto=1, pixel_minor=1, f16_store=1, N=N, Nf=Nf, frames=frames, P=P, W=W, uv=int(W == 40), xyz_al=1, uv_al=1,
                                         err_al=1, focal_ok=1, poses=1, want_err=es[0], want_soft=es[1], elem=elem))
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


@pytest.fixture(scope="module")
def sweeps():
    return [base.product(), _extra()]


def plans(lib, variant, option, cols):
    n = len(cols["N"])
    a = np.empty((n, len(IN_FIELDS)), np.int32)
    for j, f in enumerate(IN_FIELDS[1:-1]):
        a[:, j + 1] = cols[f]
    a[:, 0] = variant
    a[:, -1] = option
    out = np.empty((n, len(OUT_FIELDS)), np.int32)
    lib.k2w_plan(C.c_int64(n), a.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return {f: out[:, j] for j, f in enumerate(OUT_FIELDS)}


def has_walk(cols, p):
    """the builds with a full-tile path, from the kernel's own condition: EXF >= 2, the vector build, per-wave sums, <= 3 waves per SIMD, the grid with W % 64 == 0"""
    return (p["family"] == EXACT_VEC) & (p["exf"] >= 2) & (p["pw"] == 1) & (p["minw"] <= 3) & (cols["uv"] == 0) & (cols["W"] % 64 == 0) & (p["status"] == ref.OK)


def legal(cols, p, walk):
    hyps = 16 * np.maximum(p["ng"], 1) * walk
    return (cols["N"] % hyps == 0) & ((cols["frames"] <= 1) | (cols["Nf"] <= 0) | (cols["Nf"] % hyps == 0))


def longest_legal(cols, p, upto):
    w = np.array(upto).copy()
    for _ in range(2):
        w = np.where((w > 1) & ~legal(cols, p, w), w // 2, w)
    return w


def expected_walk(cols, p, option, auto):
    if option == 0:
        regime = (p["ch"] == 4) & (p["minw"] == 2) & (cols["N"].astype(np.float64) * cols["P"] * 4.0 > BIG_BYTES)
        w = np.where(regime, auto, 1)
        wgs = -(-cols["N"].astype(np.int64) // (16 * np.maximum(p["ng"], 1))) * -(-cols["P"].astype(np.int64) // (64 * np.maximum(p["ch"], 1)))
        for _ in range(2):
            w = np.where((w > 1) & (wgs // w < MIN_WGS), w // 2, w)
    else:
        w = np.full(len(cols["N"]), option)
    return np.where(has_walk(cols, p), longest_legal(cols, p, w), 1)


def coverage_errors(cols, p):
    """rows whose grid does not cover every hypothesis tile exactly once: walk w of the grid scores tiles w * hyp_walk ... + hyp_walk - 1"""
    ok = (p["status"] == ref.OK) & (p["ng"] > 0)
    key = np.stack([cols["N"][ok], p["ng"][ok], p["hyp_walk"][ok], p["walks"][ok]], axis=1)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    bad = np.zeros(len(uniq), bool)
    for i, (N, ng, walk, walks) in enumerate(uniq.tolist()):
        tiles = (np.arange(walks)[:, None] * walk + np.arange(walk)[None, :]).ravel()
        NT = -(-N // (16 * ng))
        bad[i] = not np.array_equal(np.sort(tiles), np.arange(NT))
    return int(bad[inv.ravel()].sum())


def straddle_errors(cols, p):
    w = p["hyp_walk"]
    return int(((w > 1) & ~legal(cols, p, w)).sum())


def test_the_walk_of_every_plan(k2w, sweeps):
    auto = k2w.k2w_auto_walk()
    assert auto in (1, 2, 4)
    seen = set()
    # the big sweep with the auto policy, every exact-form id and one id of every other family; the walk's own sweep with every id
    for cols, ids in zip(sweeps, ([-1, -2, 0, 21, 42, 58, 60, 81, 84, 85, 89, 93, 94, 95], base.IDS)):
        for v in ids:
            one = plans(k2w, v, 1, cols)
            assert (one["hyp_walk"] == 1).all()
            for option in (0, 2, 4):
                p = plans(k2w, v, option, cols)
                for f in OUT_FIELDS[:-2]:
                    assert np.array_equal(p[f], one[f]), (v, option, f)
                assert np.isin(p["hyp_walk"], (1, 2, 4)).all()
                assert (p["hyp_walk"][~has_walk(cols, p)] == 1).all(), (v, option)
                want = expected_walk(cols, p, option, auto)
                i = int(np.argmax(p["hyp_walk"] != want))
                assert np.array_equal(p["hyp_walk"], want), (v, option, {k: int(c[i]) for k, c in cols.items()}, int(p["hyp_walk"][i]), int(want[i]))
                assert straddle_errors(cols, p) == 0 and coverage_errors(cols, p) == 0, (v, option)
                seen |= {(option, int(w)) for w in np.unique(p["hyp_walk"])}
    # forced walks of 2 and 4 ran and were shortened; the auto policy left small launches alone
    assert {(2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (0, 1)} <= seen
    assert ((0, auto) in seen)


def test_the_auto_policy_leaves_one_frame_alone(k2w):
    """one 640 x 480 frame of 256 hypotheses is 2.3 fills of the chip at a walk of 1: never walked, whatever the measured length; the bench shape takes it"""
    cols = {k: np.array([v]) for k, v in dict(flags=0, exact_auto=1, pixel_minor=1, f16_store=1, N=256, Nf=0, frames=1, P=307200, W=640, uv=0, xyz_al=1, uv_al=1, err_al=1,
                                               focal_ok=1, poses=1, want_err=1, want_soft=1, elem=0).items()}
    assert plans(k2w, -1, 0, cols)["hyp_walk"][0] == 1
    cols["N"], cols["Nf"], cols["frames"] = np.array([4096]), np.array([256]), np.array([16])
    assert plans(k2w, -1, 0, cols)["hyp_walk"][0] == k2w.k2w_auto_walk()


@pytest.mark.parametrize("mistake", ["straddle_allowed", "grid_not_divided"])
def test_a_planted_mistake_is_noticed(k2w, sweeps, mistake):
    cols = sweeps[1]
    p = {k: v.copy() for k, v in plans(k2w, -1, 4, cols).items()}
    if mistake == "straddle_allowed":
        # frames of 128 hypotheses walked by 4 all the same (the grid divided accordingly)
        hit = has_walk(cols, p) & (cols["frames"] > 1) & (cols["Nf"] == 128)
        assert hit.any()
        p["hyp_walk"][hit] = 4
        p["walks"][hit] = -(-(-(-cols["N"][hit] // 64)) // 4)
        assert straddle_errors(cols, p) > 0
    else:
        hit = p["hyp_walk"] > 1
        assert hit.any()
        p["walks"][hit] = -(-cols["N"][hit] // 64)  # one workgroup per tile, each walking hyp_walk tiles
        assert coverage_errors(cols, p) > 0
