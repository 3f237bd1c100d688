"""The waits on the vector memory counter in the full-tile path of the exact K2 builds, read from the built object (scripts/isa_waits.py).

gfx950 counts loads and stores in one counter, so a wait the compiler places for an operand register drains the wave's own error-image stores.  In the
full-tile path of the bench kernel k_reproject_st<4, 4, 1, .., G64, MINW 2, EXF 2> and of its error-images-only and 16-bit twins, behind the first
error-image store there may be
   at most three waits, each at a group top (behind the partial-sum stores of the group before, in front of the group's first error-image store) and each
   leaving at least one group's error-image stores in flight: 16, or 8 in the builds whose lanes trade rows and store 16 bytes twice per chunk (EXF 4 / 6 --
   between the fetch of a group's operands and their first use that build ISSUES only 8 stores, so no correct wait can leave more),
   and none in a chunk body, at a group end or in the last group.
The sums-only twin stores no error image; its waits behind the first partial-sum store are held to the same places.

With those waits gone nothing stalls a wave behind its stores, so the path keeps its own distance: no vector instruction writes a data register of an
error-image store within three cycles behind it.  Zero cycles was measured to corrupt the stored row (in a few chunks of a launch, lanes 12-15 of every row of
16); the compiler's rule for stores of more than 8 bytes asks for one idle cycle (two on gfx940) and leaves the buffer form with a scalar offset register
out; the kernel's fence gives four.  This holds for every build with a full-tile path, both tiles.
Skipped when the object has not been built or there is no llvm-objdump."""

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "dsac_amd", "csrc", "build", "k_forward.o")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_waits  # noqa: E402

NG, CHW = 4, 4
# (ERR, SOFT, EXF) of the bench tile on the implicit grid
BUILDS = [(1, 1, x) for x in (2, 3, 4, 5, 6)] + [(1, 0, x) for x in (2, 3, 4, 5, 6)] + [(0, 1, 2)]


def _name(err, soft, exf):
    return "k_reproject_stILi%dELi%dELi1ELb1ELb%dELb%dELb0ELb1ELi2ELb0ELi%dELi0EEEv" % (NG, CHW, err, soft, exf)


@pytest.fixture(scope="module")
def code():
    if not os.path.exists(OBJ) or not os.path.exists(isa_waits.OBJDUMP):
        pytest.skip("no built k_forward.o or no llvm-objdump")
    pattern = "k_reproject_stILi%dELi%dELi1ELb1ELb[01]ELb[01]ELb0ELb1ELi2ELb0ELi[2-6]ELi0EEEv" % (NG, CHW)
    return isa_waits.kernels(isa_waits.disassemble(OBJ, pattern), pattern)


@pytest.mark.parametrize("err,soft,exf", BUILDS)
def test_full_tile_path_waits_only_at_group_tops(code, err, soft, exf):
    names = [n for n in code if _name(err, soft, exf) in n]
    assert len(names) == 1, names
    rep, _ = isa_waits.full_tile_path(code[names[0]])
    print("\n".join(isa_waits.table(names[0], rep)))
    per_group = (CHW * (2 if exf in (4, 6) else 4)) if err else 0
    # the path: every error-image store of a full tile, none of them under an exec-masked skip
    assert rep["err_stores"] == NG * per_group and rep["err_stores_under_execz"] == 0, (rep["err_stores"], rep["err_stores_under_execz"])
    other = rep["stores"] - rep["err_stores"]  # the partial-sum stores
    assert other % NG == 0 and (other > 0) == bool(soft)
    late = [w for w in rep["waits"] if (w["after_first_store"] if err else w["stores_before"] > 0)]
    assert len(late) <= NG - 1, late
    tops = set()
    for w in late:
        k, rest = divmod(w["err_stores_before"], per_group) if err else divmod(w["stores_before"], other // NG)
        assert rest == 0 and 1 <= k <= NG - 1, "a wait inside a chunk body or behind the last group: %s" % w
        assert w["stores_before"] - w["err_stores_before"] == k * (other // NG), "a wait at a group's end, in front of its partial-sum stores: %s" % w
        assert w["n"] >= per_group, "vmcnt(%d) drains the group's %d stores: %s" % (w["n"], per_group, w)
        tops.add(k)
    assert len(tops) == len(late), "two waits at one group top: %s" % late


ALL = "k_reproject_stILi4ELi[14]ELi1ELb1ELb1ELb[01]ELb0ELb1ELi[23]ELb0ELi[2-6]ELi0EEEv"


def test_no_vector_write_right_behind_a_store_of_the_full_tile_path():
    if not os.path.exists(OBJ) or not os.path.exists(isa_waits.OBJDUMP):
        pytest.skip("no built k_forward.o or no llvm-objdump")
    ks = isa_waits.kernels(isa_waits.disassemble(OBJ, ALL), ALL)
    assert len(ks) == 20, sorted(ks)  # (ERR, SOFT) in ((1, 0), (1, 1)) x EXF 2..6 x two tiles
    for name, c in sorted(ks.items()):
        rep, _ = isa_waits.full_tile_path(c)
        assert rep["err_stores"] > 0 and rep["err_stores_under_execz"] == 0, name
        bad = isa_waits.early_overwrites(c, rep["order"], 3)
        assert not bad, (name, bad[:3])
