"""CPU: the gate contract of include/cvo_frontend.h (at cvo_fe_depth_gate).  The numpy restatement
(tests/fe_gate_ref.py) against answers written by hand, the library's host-only
cvo_fe_check_depth_gate, the structure against its ctypes mirror, and the conditions the shared
(scene, gate) cases are there for, so that the GPU tests cannot pass on nothing.  The contract is
the library's own definition: PARITY UNPINNED against any SDK's filter."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fe_gate_ref as G
import fe_rectify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plane(h, w, v=1600):
    return np.full((h, w), v, np.uint16)


# ---- the restatement against answers written by hand ---------------------------------------

def test_the_jump_threshold_by_hand():
    """jump_rel = 0.0625f (exact), m = 1600: 0.0625 * 1600 = 100; D = 100 is no jump, D = 101 is one"""
    U = _plane(5, 5)
    U[2, 2] = 1700
    assert not G.jump_marks(U, 0.0625, 0).any()
    U[2, 2] = 1701
    J = G.jump_marks(U, 0.0625, 0)
    assert J[1:4, 1:4].all() and J.sum() == 9   # the centre and its eight neighbours: both sides of a step
    U = _plane(7, 7)
    U[3, 3] = 1701
    J = G.jump_marks(U, 0.0625, 0)
    want = np.zeros((7, 7), bool)
    want[2:5, 2:5] = True
    assert np.array_equal(J, want)
    # the smaller of the two is m: 1500 beside 1600 is D = 100 > 93.75, 1506 beside 1600 is D = 94 > 94.125: no
    U = _plane(5, 5)
    U[2, 2] = 1500
    assert G.jump_marks(U, 0.0625, 0)[2, 2]
    U[2, 2] = 1506
    assert not G.jump_marks(U, 0.0625, 0).any()
    # jump_rel = 0: no jump test at all
    U[2, 2] = 60000
    assert not G.jump_marks(U, 0.0, 0).any()


def test_outside_never_marks_and_a_hole_marks_only_under_hole_border():
    U = _plane(5, 6)
    assert not G.jump_marks(U, 0.05, 1).any()           # borders and corners: nothing outside marks
    U[2, 3] = 0
    assert not G.jump_marks(U, 0.05, 0).any()           # a hole is no jump
    J = G.jump_marks(U, 0.05, 1)
    want = np.zeros((5, 6), bool)
    want[1:4, 2:5] = True
    want[2, 3] = False                                  # J = 0 where U == 0
    assert np.array_equal(J, want)
    U = _plane(5, 6)
    U[0, 0] = 0                                         # a hole in the corner
    J = G.jump_marks(U, 0.0, 1)
    assert J.sum() == 3 and J[0, 1] and J[1, 0] and J[1, 1]


def test_chebyshev_reach_of_grow():
    J = np.zeros((9, 9), bool)
    J[4, 4] = True
    for g in range(4):
        want = np.zeros((9, 9), bool)
        want[4 - g:5 + g, 4 - g:5 + g] = True           # the square, corners included
        assert np.array_equal(G.near(J, g), want), g
    J = np.zeros((9, 9), bool)
    J[0, 8] = True                                      # across a corner of the image: cut, never wrapped
    for g in range(4):
        want = np.zeros((9, 9), bool)
        want[0:1 + g, 8 - g:9] = True
        assert np.array_equal(G.near(J, g), want), g


def test_range_edges_in_float32():
    """scale 5000, min_range 0.8f = 0.800000011920929: 4000 / 5000 rounds to 0.8f itself and is kept, 3999 is dropped;
    the limits are inside"""
    U = np.array([[3999, 4000, 4001, 0, 20000, 20001, 19999]], np.uint16)
    assert G.out_of_range(U, 0.8, 0.0, 5000.0).tolist() == [[True, False, False, True, False, False, False]]
    assert G.out_of_range(U, 0.0, 4.0, 5000.0).tolist() == [[False, False, False, False, False, True, False]]
    assert not G.out_of_range(U, 0.0, 0.0, 5000.0).any() and not G.out_of_range(U, -1.0, -2.0, 5000.0).any()
    dep, flags = G.gate(U, G.make_gate(0.8, 4.0), 5000.0)
    assert dep.tolist() == [[0, 4000, 4001, 0, 20000, 0, 19999]]
    assert flags.tolist() == [[G.RANGE, 0, 0, 0, 0, G.RANGE, 0]]          # (a hole has no flags)


def test_mask_and_mask_through_a_map():
    U = _plane(5, 5)
    U[0, 0] = 0
    mask = np.zeros((5, 5), np.uint8)
    mask[0, 0] = 1; mask[1, 2] = 255; mask[4, 4] = 3
    dep, flags = G.gate(U, None, 5000.0, mask)
    want = np.zeros((5, 5), np.uint8)
    want[1, 2] = want[4, 4] = G.MASKED                 # ... and none at the hole
    assert np.array_equal(flags, want) and np.array_equal(dep, np.where(want, 0, U))
    # a map that shifts by (+1.5, -1) pixels: qu = 32 u + 48 -> xn = floor((32 u + 64) / 32) = u + 2 (a tie goes up),
    # qv = 32 v - 32 -> yn = v - 1; sources outside the image count as masked
    v, u = np.mgrid[0:5, 0:5]
    qu, qv = (32 * u + 48).astype(np.int32), (32 * v - 32).astype(np.int32)
    got = G.masked_through_map(mask, qu, qv)
    want = np.zeros((5, 5), bool)
    want[0, :] = True                                   # yn = -1
    want[:, 3:] = True                                  # xn = 5, 6
    want[2, 0] = True                                   # mask[1][2]
    assert np.array_equal(got, want)
    # one fifteen-thirty-second short of the tie: xn = u + 1
    assert G.masked_through_map(mask, qu - 1, qv + 32)[1, 1] and not G.masked_through_map(mask, qu - 1, qv + 32)[1, 0]


def test_flags_are_independent_and_the_marks_ignore_range_and_mask():
    """a far pixel (5.5 m) in a plane at 1.6 m: out of range itself, and its neighbours are near a jump although the
    pixel that makes the jump is dropped by range and mask"""
    U = _plane(7, 7, 8000)
    U[3, 3] = 27500
    mask = np.zeros((7, 7), np.uint8)
    mask[3, 3] = 1
    dep, flags = G.gate(U, G.make_gate(0.8, 4.0, 0.05, 1), 5000.0, mask)
    assert flags[3, 3] == G.MASKED | G.RANGE | G.JUMP
    want = np.zeros((7, 7), np.uint8)
    want[1:6, 1:6] = G.JUMP                              # J on the 3 x 3, grown by one
    want[3, 3] = 7
    assert np.array_equal(flags, want) and np.array_equal(dep != 0, want == 0)
    # a gate whose tests are all off gates nothing
    dep, flags = G.gate(U, G.make_gate(grow=3), 5000.0)
    assert not flags.any() and np.array_equal(dep, U)


# ---- the library's host-only entry and the structure ---------------------------------------

def test_check_depth_gate_table(pkg):
    F = pkg.frontend
    L = F.lib()
    assert L.cvo_fe_check_depth_gate(None) != 0
    for g in G.good_gates():
        assert F.check_depth_gate(F.DepthGate(**g)), g
    bad = G.bad_gates()
    assert len(bad) >= 10
    for g in bad:
        assert not F.check_depth_gate(F.DepthGate(**g)), g
    # set / get without a context
    good = F.DepthGate(0.8, 4.0, 0.05, 1)
    assert L.cvo_fe_set_depth_gate(None, C.byref(good)) != 0 and L.cvo_fe_set_depth_gate(None, None) != 0
    assert L.cvo_fe_get_depth_gate(None, C.byref(good), None) != 0
    assert L.cvo_fe_set_mask(None, None, 0) != 0


def test_depth_gate_structure(pkg):
    """24 bytes, and the header's members in the header's order against the ctypes mirror"""
    F = pkg.frontend
    assert C.sizeof(F.DepthGate) == 24
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    body = re.search(r"typedef struct cvo_fe_depth_gate \{(.*?)\} cvo_fe_depth_gate;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for ctype, names in re.findall(r"\b(float|int32_t)\s+([^;]+);", body):
        members += [(n.strip(), ctype) for n in names.split(",")]
    mirror = [(n, "float" if t is C.c_float else "int32_t") for n, t in F.DepthGate._fields_]
    assert members == mirror and len(mirror) == 6
    assert [getattr(F.DepthGate, n).offset for n, _ in F.DepthGate._fields_] == [0, 4, 8, 12, 16, 20]
    g = F.DepthGate(0.8, 4.0, 0.05, 2, 1)
    assert eval(repr(g), {"DepthGate": F.DepthGate}) == g and g != F.DepthGate(0.8, 4.0, 0.05, 2, 0)
    assert g.astuple()[3:] == (2, 1)
    assert (F.STAGE_UNGATED_DEPTH, F.STAGE_GATE) == (13, 14)
    assert (F.GATE_MASKED, F.GATE_RANGE, F.GATE_JUMP) == (G.MASKED, G.RANGE, G.JUMP) == (1, 2, 4)
    for name in ("cvo_fe_set_depth_gate", "cvo_fe_get_depth_gate", "cvo_fe_check_depth_gate", "cvo_fe_set_mask"):
        assert name in F.SYMBOLS


# ---- the cases reach what they are for -----------------------------------------------------

ALL = [(name, w, h, seed) for name in G.CASES for (w, h) in G.SIZES for seed in G.SEEDS]


@pytest.mark.parametrize("name", list(G.CASES))
def test_every_enabled_rule_decides_alone_somewhere_and_a_quarter_survives(name):
    for _, w, h, seed in [c for c in ALL if c[0] == name]:
        gate, U, mask = G.case_inputs(name, w, h, seed)
        m, r, n = G.rule_planes(U, gate, G.SCALE, mask)
        valid = U != 0
        enabled = []
        if mask is not None:
            enabled.append(("mask", m, r | n))
        if gate is not None and (gate["min_range"] > 0 or gate["max_range"] > 0):
            enabled.append(("range", r, m | n))
        if gate is not None and (gate["jump_rel"] > 0 or gate["hole_border"]):
            enabled.append(("jump", n, m | r))
        assert enabled
        for rule, own, others in enabled:
            alone = np.count_nonzero(own & ~others)
            assert alone >= 1, (name, w, h, seed, rule)
        dep, flags = G.gate(U, gate, G.SCALE, mask)
        kept = np.count_nonzero(dep) / np.count_nonzero(valid)
        print(name, (w, h), seed, "kept %.2f" % kept, {k: int(np.count_nonzero(flags & k)) for k in (1, 2, 4)})
        assert kept >= 0.25 and np.count_nonzero(flags) >= 1
        if gate is not None and gate["hole_border"]:
            assert (U == 0).any()
            off = G.gate(U, dict(gate, hole_border=0), G.SCALE, mask)[1]
            assert np.count_nonzero(flags & ~off & G.JUMP) >= 1            # the hole rule decides somewhere
        if gate is not None and gate["grow"]:
            less = G.gate(U, dict(gate, grow=gate["grow"] - 1), G.SCALE, mask)[1]
            assert np.count_nonzero(flags & ~less & G.JUMP) >= 1           # ... and so does the last ring of grow


def test_the_seam_scene_steps_on_the_seams_and_the_borders():
    tw, th = G.TILE
    for w, h in G.SIZES:
        U = G.seam_scene(w, h, 72)
        J = G.jump_marks(U, 0.05, 0)
        assert J[th - 1:th + 1, :].any() and J[2 * th - 1:2 * th + 1, :].any() and J[3 * th - 1:3 * th + 1, :].any()
        assert J[0].any() and J[-1].any() and J[:, 0].any() and J[:, -1].any()
        if w > tw:
            assert J[:, tw - 1].any() and J[:, tw].any()
        assert (U[3 * th - 1] == 0).any() and (U[3 * th] == 0).any()


def test_the_scenes_have_what_the_contract_names():
    for w, h in G.SIZES:
        for seed in G.SEEDS:
            U = G.gate_scene(w, h, seed, None)
            assert U[0, 0] == 3500 and U[-1, -1] == 27500 and (U != 0).all()
            z = U.astype(np.float32) / np.float32(5000.0)
            assert (z < 0.8).any() and (z > 4.0).any()
            assert np.count_nonzero(G.gate_scene(w, h, seed, "random") == 0) >= w * h // 100
            assert np.count_nonzero(G.gate_scene(w, h, seed, "blocks") == 0) == 6 * 9 + 5 * 7


def test_the_mask_follows_a_distorting_map_somewhere():
    """under model A of the rectification tests the mask through the map differs from the mask as it is, and
    some sources lie outside the image"""
    w, h, model = R.SMALL["A"]
    qu, qv = R.rectify_map(model, w, h)
    mask = G.mask_scene(w, h, 72)
    through = G.masked_through_map(mask, qu, qv)
    assert np.count_nonzero(through != G.masked_plain(mask)) >= 10
    xn, yn = (qu.astype(np.int64) + 16) >> 5, (qv.astype(np.int64) + 16) >> 5
    assert ((xn < 0) | (xn >= w) | (yn < 0) | (yn >= h)).any()
