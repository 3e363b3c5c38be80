"""CPU: the inputs of tests/test_recon_counts_gpu.py keep the margins of the restatements, the E_cpu of the new size cases is
what is recorded, and the comparisons of that file can fail: every comparison is applied between the true restatement and a
mutant of it.  No GPU is involved.

The mutant table (which slice count catches which mutant; `-` = the mutation changes nothing there, asserted as such):

    n              63  64  65 128 129 255 256 257 300
    drop_ragged     -   -   x   -   x   x   -   x   x     the ragged last trip where it is not the first
    drop_256        -   -   -   -   -   -   -   x   x     the second thread stride, the second workgroup
    trip0_again     -   -   x   x   x   x   x   x   x     trip 0 read once more in place of trip 1
    reverse         x   x   x   x   x   x   x   x   x     caught by bit equality only: 4 * E_cpu does not see it
    compose: the columns 4 and 5 of slice 42 lost: n = 42 -, 43 x, 44 x, 300 x
"""
import math

import numpy as np
import pytest

from tests import util_imatch64 as IM
from tests import util_recon_counts as RC
from tests import util_robust64 as RB
from tests import util_svr_group64 as GU

F32, F64 = np.float32, np.float64
TABLE = {  # mutant: the counts at which it changes anything
    "drop_ragged": (65, 129, 255, 257, 300),
    "drop_256": (257, 300),
    "trip0_again": (65, 128, 129, 255, 256, 257, 300),
    "reverse": RC.COUNTS,
}


def test_the_counts_and_the_table_are_what_the_walks_make_them():
    assert RC.COUNTS == (63, 64, 65, 128, 129, 255, 256, 257, 300) and set(TABLE) == set(RB.ORDER_MUTANTS)
    for mutant, active in TABLE.items():
        for n in RC.COUNTS:
            same = np.array_equal(RB.slice_order(n, mutant), np.arange(n))
            assert same == (n not in active), (mutant, n)
    assert RB.slice_order(300, "drop_ragged").tolist() == list(range(256)) and RB.slice_order(65, "drop_256").tolist() == list(range(65))
    assert RB.slice_order(130, "trip0_again").tolist() == list(range(64)) + list(range(64)) + [128, 129]


# ---- the inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RC.COUNTS)
def test_count_cases_keep_the_margins_and_populate_both_classes(n):
    c = RC.robust_case(n)
    S = RC.robust_em(c)
    assert RB.MARGIN <= S["margin"] < math.inf and not S["frozen"].any()
    dead = RC.not_ok_slices(n)
    ws = S["ws"][-1]
    assert not ws[dead].any() and (S["rows"][dead, 0] == 3).all() and 7 in dead and n - 1 in dead and (n <= 256 or 256 in dead)
    rejected = np.flatnonzero(ws < 0.5)  # about a tenth of the slices are corrupted
    assert len(rejected) - len(dead) >= max(n // 20, 2) and ((ws > 0.01) & (ws < 0.99)).any() and (ws == 1).sum() > n // 2
    so = (1.0 - S["ws"][-2])[S["rows"][:, 0] >= 4].sum()
    assert so > 0  # the outlier class has mass, so mu2 is its mean and not the fallback
    # slice k differs from slice k + 64 and from slice k + 256, in its inputs and in its row
    for step in (64, 256):
        if n > step:
            a, b = S["rows"][:n - step], S["rows"][step:]
            live = (a[:, 0] >= 4) & (b[:, 0] >= 4)
            assert (np.abs(a - b)[live][:, [2, 4, 5]] > 0).all()
    m = RC.imatch_case(n)
    M = RC.imatch_run(m)
    IM.assert_margin(M)
    assert M["frozen"] == 0 and not M["ok"][dead].any() and M["ok"].sum() == n - len(dead)
    assert len(np.unique(M["raw"][M["ok"]])) == n - len(dead) and M["rows"][n - 1, 4] == M["rows"][:, 4].max()
    assert S["rows"][n - 1, 5] == S["rows"][:, 5].max()  # the last slice holds max y in both units


def test_the_two_late_cases_meet_their_condition_in_slice_270_alone():
    c = RC.robust_freeze_case()
    rows = RC.robust_rows32(c)
    assert np.isinf(rows[RC.LATE, 2]) and np.isfinite(np.delete(rows, RC.LATE, 0)).all() and RC.LATE >= 256
    for mutant, frozen in ((None, 1), ("reverse", 1), ("drop_256", 0), ("drop_ragged", 0)):
        S = RB.update(RB.new_state(300, 1), 0, rows, mutant=mutant)
        assert S["frozen"][0] == frozen, mutant
    assert not RB.update(RB.new_state(300, 1), 0, RC.robust_rows32(RC.robust_case(300)))["frozen"][0]
    b = RC.imatch_bad_case()
    rows = RC.imatch_rows32(b)
    S = IM.scale(rows)
    assert S["frozen"] == 1 and 0 < S["raw"][RC.LATE] < 1e-46 and np.isfinite(rows).all()
    assert F32(S["raw"][RC.LATE] / np.delete(S["raw"], RC.LATE).mean()) == 0  # the scale that leaves fp32
    assert IM.scale(np.delete(rows, RC.LATE, 0))["frozen"] == 0 and IM.scale(RC.imatch_rows32(RC.imatch_case(300)))["frozen"] == 0


def test_size_cases_reach_the_paths_they_are_named_for():
    hw = [h * w for h, w in RC.SIZES]
    assert hw == [1, 2, 6, 1024, 1026, 1028, 3075]
    assert 6 % 4 == 2 and 1026 % 4 == 2 and 1026 - 1024 == 2 and 1024 % 4 == 0 and 1028 % 4 == 0 and 1028 - 1024 == 4
    assert -(-3075 // RB.CHUNK) == 4 and -(-1024 // RB.CHUNK) == 1 and -(-1028 // RB.CHUNK) == 2
    for shape in RC.SIZES:
        c, m = RC.robust_size_case(shape), RC.imatch_size_case(shape)
        assert c["y"].shape == (3, *shape) == m["y"].shape
        S, M = RC.robust_em(c, n_em=RC.SIZE_N_EM), RC.imatch_run(m)
        if shape[0] * shape[1] < 4:
            assert S["frozen"].all() and not S["ws"].any() and M["frozen"] == 1
        else:
            assert RB.MARGIN <= S["margin"] < math.inf and not S["frozen"].any() and S["ws"][-1].tolist() == [1, 0, 1]
            assert M["frozen"] == 0 and M["ok"].all()


def test_e_cpu_of_the_size_cases_is_what_is_recorded():
    rb, im, who = RC.measure_size_e_cpu()  # asserts the margin of every size case
    print(rb, im, who)
    for g in RB.GROUPS:
        assert rb[g] <= RB.E_CPU[g], (g, rb[g])  # no robust group exceeds the recorded figure
    for g in IM.GROUPS:
        if g in IM.E_CPU_SIZES:
            assert IM.E_CPU[g] < 0.98 * IM.E_CPU_SIZES[g] <= im[g] <= IM.E_CPU_SIZES[g], (g, im[g])
        else:
            assert im[g] <= IM.E_CPU[g], (g, im[g])
    assert who["im_rows"] == (2, 513) and who["im_scale"] == (2, 513)


def test_e_cpu_of_the_bias_path_at_257_slices_is_what_is_recorded():
    c = RC.imatch_means_case()
    a, b = RC.imatch_run(c, F32, RC.MEANS_SIGMA), RC.imatch_run(c, F64, RC.MEANS_SIGMA)
    IM.assert_margin(b)
    assert b["margin"] < math.inf and a["frozen"] == b["frozen"] == 0 and np.array_equal(a["ok"], b["ok"]) and np.array_equal(a["inb"], b["inb"])
    assert b["ok"][256] and b["inb"][256].any() and np.abs(b["mean"][[0, 255, 256]]).min() > 0
    err = IM.compare(a, b)
    print(err)
    for g in IM.GROUPS:
        if g in IM.E_CPU_N257:
            assert IM.E_CPU[g] < 0.98 * IM.E_CPU_N257[g] <= err[g] <= IM.E_CPU_N257[g], (g, err[g])
        else:
            assert err[g] <= IM.E_CPU[g], (g, err[g])


# ---- the mutants: the comparisons of points 1 and 4 can fail -----------------------------------------------------------------
@pytest.mark.parametrize("n", RC.COUNTS)
def test_point_1_fails_on_every_mutant_that_changes_anything(n):
    c, m = RC.robust_case(n), RC.imatch_case(n)
    none, A = RC.robust_point1(c, None)
    assert none == set() and not A["frozen"].any()
    assert RC.imatch_point1(m, None)[0] == set()
    for mutant, active in TABLE.items():
        rb, im = RC.robust_point1(c, mutant)[0], RC.imatch_point1(m, mutant)[0]
        print(n, mutant, sorted(rb), sorted(im))
        if n in active:
            assert rb and im, (mutant, n)
        else:
            assert not rb and not im, (mutant, n)


@pytest.mark.parametrize("n", (63, 300))
def test_the_reverse_order_is_seen_by_bit_equality_and_not_by_four_e_cpu(n):
    c = RC.robust_case(n)
    a, b = RC.robust_em(c, mutant="reverse"), RC.robust_em(c)
    err = RB.compare(a, b)
    print(n, err)
    assert max(err.values()) > 0  # the sums do differ
    for g in RB.GROUPS:
        assert err[g] <= 4 * RB.E_CPU[g], (g, err[g])  # and the rule of the comparison tests lets them pass
    assert "reverse" in TABLE and RC.robust_point1(c, "reverse")[0]
    rows = RC.imatch_rows32(RC.imatch_case(n))
    A, B = IM.scale(rows), IM.scale(rows, mutant="reverse")
    d = max(IM._rel(B[k], A[k]) for k in ("scale", "raw", "consts"))
    assert d <= 4 * IM.E_CPU["scale"] and RC.differing(RC.imatch_fields(A), RC.imatch_fields(B))


@pytest.mark.parametrize("n", RC.COUNTS)
def test_point_4_svr_update_fails_on_the_workgroup_mutants(n):
    seq, theta0 = RC.hand_sequences(n)
    true = RC.svr_update_run(seq, theta0)
    assert RC.differing(true, RC.svr_update_run(seq, theta0)) == []
    for mutant in ("drop_ragged", "drop_256", "trip0_again"):
        diff = RC.differing(true, RC.svr_update_run(seq, theta0, mutant))
        assert bool(diff) == (n in TABLE[mutant]), (mutant, n, diff)
    assert RC.differing(true, RC.svr_update_run(seq, theta0, "reverse")) == []  # no sum over the slices: nothing to reverse


@pytest.mark.parametrize("n,caught", ((42, False), (43, True), (44, True), (300, True)))
def test_point_4_compose_fails_on_the_252_thread_layout(n, caught):
    base, group, phi = RC.compose_inputs(n, 3)
    gm, gj = GU.group_operands(phi, F32)
    true, mut = GU.compose(gm, gj, base, group, F32), RC.compose_mutant(gm, gj, base, group)
    same = np.array_equal(true[0].view(np.uint32), mut[0].view(np.uint32)) and np.array_equal(true[1].view(np.uint32), mut[1].view(np.uint32))
    assert same == (not caught)
    assert n <= 42 or (0 <= group[42] < 3)
    ids = set(group.tolist())
    assert ids <= {-1, 0, 1, 2, 7} and len(ids) >= 4


def test_group_reduce_inputs_cross_the_boundary_with_every_odd_member():
    for G in (8, 9, 300):
        stats, members, offsets = RC.reduce_inputs(300, G)
        assert len(offsets) == G + 1 and offsets[1] == offsets[2] and -1 in members and 300 in members  # group 1 is empty
        assert (G * 32 > 256) == (G > 8) and list(members[:6]) == [4, -1, 0, 300, 2, 4] and offsets[-1] == len(members) <= 65535
