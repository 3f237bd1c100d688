"""dk::k2_plan (dsac_amd/csrc/k2_plan.h) -- the host function that decides, before anything is enqueued, which K2 kernel scores a frame -- against an
independent restatement of the policy (tests/k2_plan_ref.py, written from the launch code the plan replaced).  The header is compiled with g++ alone
(tests/helpers/k2_plan_host.cpp): no HIP, no GPU.  Every field of every plan of the cross product below must equal the restatement; four one-line mistakes
planted in the restatement must each be noticed; no plan writes more partial-sum rows than soft_part is sized for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import k2_plan_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))

IN_FIELDS = ("variant", "flags", "exact_auto", "pixel_minor", "f16_store", "N", "Nf", "frames", "P", "W", "uv", "xyz_al", "uv_al", "err_al", "focal_ok", "poses",
             "want_err", "want_soft", "elem")
IDS = ref.KNOWN + [-1, 63, 64, 78, 99, -2]
BIT = lambda *k: sum(1 << i for i in k)
FLAGS = [0] + [BIT(i) for i in (0, 1, 5, 24, 25, 26, 27, 28, 29)] + [BIT(27, 28), BIT(25, 29), BIT(28, 29)]
# (P, W, uv): 40 x 40 with sampled positions; 53 x 37 (odd) on the grid; a 64-wide grid; P % 8 != 0 on a grid whose width is no multiple of 4; either side of
# the exact forms' tile switch; 640 x 480
MAPS = [(1600, 40, 1), (1961, 53, 0), (4096, 64, 0), (1604, 401, 0), (16384, 128, 0), (16388, 68, 0), (307200, 640, 0)]
# 815 | 816 and 3581 | 3582 hypotheses: either side of 1.0e9 and 4.4e9 bytes of error images at 307 200 cells; 156 250 x 1600 x 4 bytes are 1.0e9 exactly
N_ALL, N_AT = [1, 128, 256, 4096], {307200: [815, 816, 3581, 3582], 1600: [156250]}
ALIGN = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)]  # xyz, uv, err: each off the 16-byte grid in turn
ERR_SOFT = [(1, 0), (0, 1), (1, 1), (0, 0)]
FRAMES = [(1, 0), (2, 128)]  # (frames, Nf)


@pytest.fixture(scope="module")
def k2p(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("k2p") / "libk2p.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "helpers", "k2_plan_host.cpp")])
    lib = C.CDLL(out)
    assert lib.k2p_in_fields() == len(IN_FIELDS) and lib.k2p_out_fields() == len(ref.FIELDS)
    return lib


def product(knobs=((1, 1),), flags=FLAGS, n_all=N_ALL, n_at=N_AT):
    """the cross product as a dict of columns (without `variant`)"""
    n_list = list(n_all) + [n for v in n_at.values() for n in v]
    axes = [len(flags), 2, 2, len(ERR_SOFT), 3, len(MAPS), len(ALIGN), 2, len(n_list), len(FRAMES), len(knobs)]
    ix = [a.ravel() for a in np.indices(axes)]
    maps, align, es, fr, kn = (np.array(t)[i] for t, i in ((MAPS, ix[5]), (ALIGN, ix[6]), (ERR_SOFT, ix[3]), (FRAMES, ix[9]), (knobs, ix[10])))
    N = np.array(n_list)[ix[8]]
    cols = dict(flags=np.array(flags)[ix[0]], exact_auto=ix[1], poses=ix[2], want_err=es[:, 0], want_soft=es[:, 1], elem=ix[4], P=maps[:, 0], W=maps[:, 1],
                uv=maps[:, 2], xyz_al=align[:, 0], uv_al=align[:, 1], err_al=align[:, 2], focal_ok=ix[7], N=N, frames=fr[:, 0], Nf=fr[:, 1], pixel_minor=kn[:, 0],
                f16_store=kn[:, 1])
    keep = np.ones(len(N), bool)
    for n in set(n_list) - set(n_all):
        keep &= (N != n) | np.isin(cols["P"], [p for p, v in n_at.items() if n in v])
    return {k: v[keep] for k, v in cols.items()}


@pytest.fixture(scope="module")
def walk():
    return product()


def cxx_plans(lib, variant, cols):
    n = len(cols["N"])
    a = cols.get("_rows")  # the input rows, kept with the columns: only the id changes from call to call
    if a is None:
        a = cols["_rows"] = np.empty((n, len(IN_FIELDS)), np.int32)
        for j, f in enumerate(IN_FIELDS[1:]):
            a[:, j + 1] = cols[f]
    a[:, 0] = variant
    out = np.empty((n, len(ref.FIELDS)), np.int32)
    lib.k2p_plan(C.c_int64(n), a.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def ref_plans(variant, cols, mutant=None):
    r = ref.plan(variant, mutant=mutant, **{k: v for k, v in cols.items() if k != "_rows"})
    return np.stack([r[f] for f in ref.FIELDS], axis=1)


def first_difference(variant, cols, got, want):
    i = int(np.argmax((got != want).any(axis=1)))
    return "k2_variant %d, %s:\n  plan        %s\n  restatement %s" % (variant, {k: int(v[i]) for k, v in cols.items() if k != "_rows"}, dict(zip(ref.FIELDS, got[i].tolist())),
                                                                     dict(zip(ref.FIELDS, want[i].tolist())))


def test_every_field_of_every_plan_equals_the_restatement(k2p, walk):
    cols = walk
    assert len(cols["N"]) > 200000
    seen_forms, seen_fams, seen_status, seen_why = set(), set(), set(), set()
    for v in IDS:
        got, want = cxx_plans(k2p, v, cols), ref_plans(v, cols)
        assert np.array_equal(got, want), first_difference(v, cols, got, want)
        seen_forms |= set(np.unique(got[:, 1]).tolist()); seen_fams |= set(np.unique(got[:, 3]).tolist()); seen_status |= set(np.unique(got[:, 0]).tolist()); seen_why |= set(np.unique(got[:, 2]).tolist())
    # the walk reaches every form, every kernel family, both refusals and every reason bit
    assert seen_forms == set(range(7)) and seen_fams == set(range(10)) and seen_status == {ref.OK, ref.INVALID, ref.NOT_SUPPORTED}
    assert all(any(w & bit for w in seen_why) for bit in (1, 2, 4, 8))


def test_the_block_order_and_the_store_layout_knobs(k2p):
    """"k2_order" 0 and "k2_f16_store" 0, which the big walk leaves at their defaults: on the one-frame cases of 256 hypotheses"""
    cols = product(knobs=((0, 1), (1, 0), (0, 0)), n_all=[256], n_at={})
    cols = {k: v[cols["frames"] == 1] for k, v in cols.items()}
    for v in IDS:
        got, want = cxx_plans(k2p, v, cols), ref_plans(v, cols)
        assert np.array_equal(got, want), first_difference(v, cols, got, want)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_a_one_line_mistake_in_the_restatement_is_noticed(k2p, walk, mutant):
    """threshold_ge: a size threshold compared with >= instead of > (noticed at 1.0e9 bytes exactly);  split_for_forced_fp32: need_split true in front of a forced
    fp32 kernel;  any_tail_row_forgotten: the any-map build's extra partial row;  f16_without_p8: the 16-bit backstop accepting P % 8 != 0"""
    cols = walk
    differ = 0
    for v in (-1, 42):
        differ += int((cxx_plans(k2p, v, cols) != ref_plans(v, cols, mutant)).any(axis=1).sum())
    assert differ > 0, mutant


def test_the_id_list_is_the_one_the_launch_switch_had(k2p):
    for v in range(-4, 200):
        assert bool(k2p.k2p_variant_known(v)) == ref.known(v), v
    assert [v for v in range(200) if k2p.k2p_variant_known(v)] == ref.KNOWN


def test_no_plan_writes_more_rows_than_soft_part_holds(k2p):
    """callers size soft_part with reproject_num_pixel_tiles(P): every id and every arithmetic form on every P up to 5000 and around the sizes in use"""
    Ps = np.array(list(range(1, 5001)) + [16383, 16384, 16385, 16388, 65535, 65536, 76800, 307199, 307200, 307201, 2073600, 2073601])
    bound = np.array([k2p.k2p_num_pixel_tiles(int(p)) for p in Ps])
    assert np.array_equal(bound, ref.num_pixel_tiles(Ps))
    launched = 0
    for flags in (0, BIT(25), BIT(27), BIT(28), BIT(29)):
        for uv, W in ((1, 1), (0, 4)):
            cols = dict(flags=flags, exact_auto=1, pixel_minor=1, f16_store=1, N=4096, Nf=0, frames=1, P=Ps, W=W, uv=uv, xyz_al=1, uv_al=1, err_al=1, focal_ok=1, poses=1,
                        want_err=1, want_soft=1, elem=0)
            cols = {k: np.broadcast_to(np.asarray(v), Ps.shape) for k, v in cols.items()}
            for v in ref.KNOWN + [-1]:
                got = cxx_plans(k2p, v, cols)
                ok = got[:, 0] == ref.OK
                launched += int(ok.sum())
                tiles = got[:, ref.FIELDS.index("tiles")]
                assert (tiles[ok] >= 1).all() and (tiles[ok] <= bound[ok]).all(), (v, flags, int(Ps[ok][np.argmax(tiles[ok] - bound[ok])]))
    assert launched > 1000000


def test_the_exact_only_options_are_reported_in_the_order_of_the_messages(k2p):
    """k2_exact_only: what k2_f16_check / k2_cams_check refuse by name and the plan's 16-bit backstop refuses by status -- variant first, then flags, then
    k2_exact_auto"""
    E, A = BIT(28), BIT(29)
    for variant, flags, auto, want in ((-1, 0, 1, 0), (-1, E, 0, 0), (-1, A, 0, 0), (-1, E | A, 1, 0), (84, BIT(25), 0, 1), (0, 0, 1, 1), (-2, 0, 1, 1),
                                       (-1, BIT(25), 0, 2), (-1, E | 1, 1, 2), (-1, BIT(24), 1, 2), (-1, 0, 0, 3)):
        assert k2p.k2p_exact_only(variant, flags, auto) == want, (variant, flags, auto)
