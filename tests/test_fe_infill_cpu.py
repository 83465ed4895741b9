"""CPU: the restatement of the infill contract (tests/fe_infill_ref.py) against itself -- the loop over runs in Python
integers against the vectorised form -- what the planes made on purpose reach, and which errors of a device
implementation (tests/fe_infill_mutants.py) they tell from the restatement, each by a named plane at named settings.
No GPU: tests/test_gpu_fe_infill.py holds k_fe_infill to the same restatement by bytes."""
import numpy as np
import pytest

import fe_infill_mutants as M
import fe_infill_ref as K


def _same(a, b):
    return all(np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for p, q in zip(a, b))


@pytest.mark.parametrize("name", K.MADE_NAMES)
def test_the_loop_over_runs_equals_the_vectorised_form(name):
    for f in K.SETTINGS:
        assert _same(K.infill(K.plane(name), f), K.infill_loop(K.plane(name), f)), (name, f)


def test_the_settings_grid_and_the_sizes():
    assert set(K.GAPS) == {(0, 0), (1, 0), (0, 1), (2, 5), (15, 0), (0, 31), (15, 31)} and K.JUMPS == [0.0, 0.25]
    assert len(K.SETTINGS) == 14 and K.SIZES == [(96, 64), (127, 193)]
    for w, h in K.SIZES:
        assert w % K.TILE[0] and w > K.TILE[0] and h > K.TILE[1]     # (64 rows are four whole tiles; 193 are not)
    assert 193 % K.TILE[1]
    assert {g for gap in K.GAPS for g in gap if g} | {g + 1 for gap in K.GAPS for g in gap if g} == set(K.LENGTHS)


def test_the_value_is_what_the_contract_says():
    assert K.value(1, 2, 1, 1) == 1                       # (linear in depth, rounded half up: 2)
    assert K.value(1, 3, 1, 1) == 2                       # (a floor: 1)
    assert (K.value(3, 6, 1, 2), K.value(3, 6, 2, 1)) == (4, 5)     # (the weights swapped: 5, 4)
    assert K.value(65535, 65535, 16, 16) == 65535 and 65535 * 65535 * 32 >= 1 << 32
    assert K.value(1, 65535, 1, 1) == 2
    assert K.value(4000, 5000, 1, 1) == 4444
    assert not K.refused(4000, 5000, 0.25) and K.refused(4000, 5001, 0.25) and not K.refused(1, 65535, 0.0)
    rng = np.random.default_rng(3)
    A, B = rng.integers(1, 65536, 4000), rng.integers(1, 65536, 4000)
    da = rng.integers(1, 32, 4000)
    db = rng.integers(1, 33 - da)
    v = K.value(A, B, da, db)
    assert (v >= np.minimum(A, B)).all() and (v <= np.maximum(A, B)).all() and (v >= 1).all()
    exact = [(int(a) * int(b) * int(p + q) * 2 + int(a * p + b * q)) // (2 * int(a * p + b * q)) for a, b, p, q in zip(A, B, da, db)]
    assert v.tolist() == exact


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
def test_runs_of_g_are_bridged_and_runs_of_g_plus_one_are_not(size):
    """row-runs and col-runs: with the other pass off, exactly the runs of at most g pixels are filled, two of every
    length (four down the columns of the higher plane), one of them across the seam"""
    w, h = size
    rows, cols = K.plane("row-runs-%dx%d" % size), K.plane("col-runs-%dx%d" % size)
    assert any((rows[y, 63] == 0) and (rows[y, 64] == 0) for y in range(h))
    assert any((cols[15, x] == 0) and (cols[16, x] == 0) for x in range(w))
    copies = 2 if h > 66 else 1
    for gx, gy, j in K.SETTINGS:
        if gy == 0:
            F, flags, nr, nc = K.infill(rows, (gx, gy, j))
            assert (nr, nc) == (2 * sum(L for L in K.LENGTHS if L <= gx), 0), (gx, nr)
            for y in range(h):
                holes = int(np.count_nonzero(rows[y] == 0))
                assert int(np.count_nonzero(F[y] == 0)) == (0 if holes <= gx else holes)
        if gx == 0:
            F, flags, nr, nc = K.infill(cols, (gx, gy, j))
            assert (nr, nc) == (0, 2 * copies * sum(L for L in K.LENGTHS if L <= gy)), (gy, nc)
    print("row-runs", size, "rows of lengths", K.LENGTHS, "twice each")


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
def test_a_run_that_touches_a_border_stays_a_hole(size):
    w, h = size
    S = K.plane("borders-%dx%d" % size)
    for f in ((1, 0, 0.0), (15, 0, 0.25), (0, 1, 0.0), (0, 31, 0.25)):
        F, flags, nr, nc = K.infill(S, f)
        if f[0]:
            assert (F[:, 0][S[:, 0] == 0] == 0).all() and (F[:, w - 1][S[:, w - 1] == 0] == 0).all()
            assert np.count_nonzero(S[:, 0] == 0) == np.count_nonzero(S[:, w - 1] == 0) == 2
            assert F[7, 1] != 0 and F[11, w - 2] != 0 and flags[7, 1] == K.ROW      # one pixel away: bridged
        else:
            assert (F[0][S[0] == 0] == 0).all() and (F[h - 1][S[h - 1] == 0] == 0).all()
            assert np.count_nonzero(S[0] == 0) == np.count_nonzero(S[h - 1] == 0) == 2
            assert F[1, 22] != 0 and F[h - 2, 26] != 0 and flags[1, 22] == K.COL
        assert nr + nc >= 4


def test_the_jump_pairs():
    """4000|5000 is bridged and 4000|5001 refused at 0.25, in both orders, in a row and in a column"""
    for name in ("jumps-96x64", "jumps-127x193"):
        S = K.plane(name)
        for f, want in (((1, 0, 0.25), (2, 0, 2)), ((1, 0, 0.0), (4, 0, 0)), ((0, 1, 0.25), (0, 2, 2)), ((0, 1, 0.0), (0, 4, 0))):
            F, flags, nr, nc = K.infill(S, f)
            assert (nr, nc, int(np.count_nonzero(flags == K.JUMP))) == want, (name, f)
            assert set(F[flags != 0].tolist()) <= ({0, 4444} if f[2] else {4444, 4445})
        F, flags, nr, nc = K.infill(S, (1, 0, 0.25))
        assert [int(flags[1 + 2 * k, 4 + 9 * k if k % 2 == 0 else 64]) for k in range(4)] == [K.ROW, K.ROW, K.JUMP, K.JUMP]


def test_the_arithmetic_patterns():
    for name in ("arithmetic-96x64", "arithmetic-127x193"):
        S = K.plane(name)
        F = K.infill(S, (15, 0, 0.0))[0]
        assert F[1, 4] == 1 and F[3, 64] == 2 and (F[5, 22], F[5, 23]) == (4, 5) and F[7, 64] == 2
        assert (F[9, 39:56] == 65535).all() and S[9, 40] == 0
        F, flags, nr, nc = K.infill(S, (0, 31, 0.0))
        assert (F[12:45, 60] == 65535).all() and (flags[13:44, 60] == K.COL).all() and nc >= 31 + 15 + 5
        flags = K.infill(S, (15, 0, 0.25))[1]
        assert flags[7, 64] == K.JUMP and flags[3, 64] == K.JUMP and flags[1, 4] == K.JUMP and flags[5, 22] == K.JUMP


def test_the_column_pass_reads_h_and_no_pass_is_in_place():
    for size in ("96x64", "127x193"):
        S = K.plane("columns-read-h-" + size)
        F, flags, nr, nc = K.infill(S, (2, 5, 0.0))
        assert (nr, nc) == (3, 3)
        for x, y in ((20, 4), (63, 15), (72, 14)):
            assert S[y, x] == 0 and F[y, x] == 4190 and flags[y, x] == K.ROW
            assert F[y + 1, x] == K.value(4190, 4100, 1, 1) and flags[y + 1, x] == K.COL
        S = K.plane("not-in-place-" + size)
        F, flags, nr, nc = K.infill(S, (2, 0, 0.0))
        assert F[1, 3:7].tolist() == [4000, 4286, 4615, 5000] and nr == 4
        assert K.value(4286, 5000, 1, 1) == 4616                 # (what a sweep in place makes of the second hole)


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_ground_plane_is_met_within_one_unit(size):
    """every filled ground pixel is within 1 unit of the plane's true rounded depth; linear in depth is off by more
    than 100 units"""
    w, h = size
    S, (truth, rows) = K.plane("ground-%dx%d" % size), K.ground_truth(w, h)
    clear = K.ground_pixels(w, h)
    for f in K.SETTINGS:
        F, flags, nr, nc = K.infill(S, f)
        filled = ((flags == K.ROW) | (flags == K.COL)) & clear
        err = np.abs(F.astype(np.int64) - truth)[filled]
        print("ground", size, f, "filled ground pixels", err.size, "worst", err.max() if err.size else None)
        assert err.size == 0 or err.max() <= 1
        if f[1] >= 4:
            assert err.size >= 0.4 * np.count_nonzero(truth) and np.count_nonzero(flags == K.COL) >= 1000
            assert (f[2] == 0) == (np.count_nonzero(flags == K.JUMP) == 0)      # the poles: refused at 0.25
    F, flags = M.linear(S, (2, 5, 0.0))[:2]
    filled = ((flags == K.ROW) | (flags == K.COL)) & clear
    worst = int(np.abs(F.astype(np.int64) - truth)[filled].max())
    print("ground", size, "linear in depth: worst", worst)
    assert worst > 100


def test_every_flag_value_occurs_and_runs_are_refused():
    for name in ("sparse-96x64", "sparse-127x193", "ground-96x64", "jumps-96x64"):
        flags = K.made(name, (2, 5, 0.25))[2]
        counts = {int(v): int(np.count_nonzero(flags == v)) for v in (0, K.ROW, K.COL, K.JUMP)}
        print(name, "flags", counts)
        assert min(counts.values()) >= 1 and sum(counts.values()) == flags.size
    S, F, flags, nr, nc = K.made("sparse-127x193", (15, 31, 0.25))
    assert (F[S != 0] == S[S != 0]).all() and (flags[S != 0] == 0).all()      # a pixel with a depth is never changed
    assert (S == 65535).any() and (S == 1).any()


# ---- the mutants ---------------------------------------------------------------------------------------

TOLD = [(M.linear, "arithmetic-96x64", (1, 0, 0.0)), (M.floor, "arithmetic-96x64", (1, 0, 0.0)),
        (M.weights_swapped, "arithmetic-96x64", (15, 0, 0.0)), (M.product_32, "arithmetic-96x64", (15, 0, 0.0)),
        (M.sum_for_length, "row-runs-96x64", (1, 0, 0.0)), (M.per_side, "row-runs-96x64", (15, 0, 0.0)),
        (M.border_end, "borders-96x64", (1, 0, 0.0)), (M.not_strict, "jumps-96x64", (1, 0, 0.25)),
        (M.relative_to_hi, "jumps-96x64", (0, 1, 0.25)), (M.columns_on_s, "columns-read-h-96x64", (2, 5, 0.0)),
        (M.columns_first, "columns-read-h-96x64", (2, 5, 0.0)), (M.in_place, "not-in-place-96x64", (15, 0, 0.0)),
        (M.limits_swapped, "row-runs-96x64", (15, 0, 0.0)), (M.limits_swapped, "col-runs-96x64", (0, 31, 0.0))]
NOT_TOLD = [(M.weights_swapped, "jumps-96x64", (1, 0, 0.0), "da = db in a hole of one pixel"),
            (M.product_32, "jumps-96x64", (1, 0, 0.0), "4000 * 5001 * 2 is below 2^32"),
            (M.not_strict, "jumps-96x64", (1, 0, 0.0), "no test at jump_rel 0"),
            (M.relative_to_hi, "jumps-96x64", (0, 1, 0.0), "no test at jump_rel 0"),
            (M.limits_swapped, "sparse-96x64", (0, 0, 0.25), "both limits 0"),
            (M.columns_on_s, "sparse-96x64", (15, 0, 0.25), "no column pass"),
            (M.columns_first, "sparse-96x64", (0, 31, 0.25), "no row pass")]


@pytest.mark.parametrize("mutant,name,f", TOLD, ids=["%s-%s-%s" % (m.__name__, n, "-".join(map(str, f))) for m, n, f in TOLD])
def test_a_made_plane_tells_the_mutant_from_the_restatement(mutant, name, f):
    want, got = K.made(name, f)[1:], mutant(K.plane(name), f)
    assert not np.array_equal(want[0], got[0]), "%s: F equals the restatement's on %s at %s" % (mutant.__name__, name, f)


@pytest.mark.parametrize("mutant,name,f,why", NOT_TOLD, ids=["%s-%s" % (m.__name__, n) for m, n, f, w in NOT_TOLD])
def test_where_a_mutant_cannot_differ_it_does_not(mutant, name, f, why):
    assert _same(K.made(name, f)[1:], mutant(K.plane(name), f)), why


def test_linear_equals_the_contract_between_equal_ends():
    S = np.array([[7, 0, 0, 7, 9, 65535, 0, 0, 0, 65535]], np.uint16)
    assert _same(K.infill(S, (3, 0, 0.0)), M.linear(S, (3, 0, 0.0)))


@pytest.mark.parametrize("tile", M.TILES, ids=lambda t: "%dx%d" % t)
def test_a_lost_halo_shows(tile):
    """ends lost at the borders of tiles of 64 x 16, 32 x 8, 16 x 16 and 64 x 4: on the runs across the seams and on the
    sparse plane, at the settings the GPU test compares"""
    for name, f in (("row-runs-96x64", (15, 0, 0.0)), ("col-runs-96x64", (0, 31, 0.0)), ("sparse-96x64", (2, 5, 0.25)),
                    ("sparse-127x193", (15, 31, 0.0)), ("columns-read-h-96x64", (2, 5, 0.0))):
        want, got = K.made(name, f)[1:], M.tile_cut(K.plane(name), f, *tile)
        assert not np.array_equal(want[0], got[0]), (name, f, tile)
