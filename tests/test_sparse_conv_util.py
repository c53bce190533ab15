"""CPU: the reference and the bound of the single-layer sparse convolution tests (sparse_conv_util.py) are sharp enough to catch a
subtly wrong kernel — a dropped (row, tap) entry, an entry that reads the neighbouring input row, a lost input channel each move the
touched row by far more than the tolerance — and the reference means what the encoder's oracle means by a neighbour table."""
import numpy as np
import pytest

import sparse_conv_util as SC
from util import cases, hashfill
from oracle import sparse_encoder_ref as SR


def _rows_ref(case, rows, feats=None, nbr=None):
    """reference of some rows of a case (rows are independent), with the features or the table replaced"""
    d = SC.inputs(case)
    add = d["add"][rows] if d["add"] is not None else None
    return SC.reference(d["feats"] if feats is None else feats, (d["nbr"] if nbr is None else nbr)[rows], d["w"], d["scale"], d["bias"], case.act, add,
                        case.add == "pre")


def _probes(case, k=24):
    """(row, tap) positions with a live entry, spread over the table by a hash (every live entry of a small table)"""
    nbr = SC.inputs(case)["nbr"]
    r, t = np.nonzero(nbr >= 0)
    if len(r) <= k:
        return list(zip(r.tolist(), t.tolist()))
    pick = np.unique((hashfill.uniform01("sc_probe_" + case.name, k, 2) * len(r)).astype(np.int64))
    return list(zip(r[pick].tolist(), t[pick].tolist()))


@pytest.mark.parametrize("case", [SC.SMALLEST, SC.LARGEST], ids=lambda c: c.name)
def test_mutations_of_the_reference_exceed_the_bound(case):
    d = SC.inputs(case)
    ref, tol = SC.expected(case)
    assert case.act == "none"      # a ReLU could hide a mutation behind a clamped output; the sharpness is shown on the linear cases
    margins = {"dropped entry": [], "neighbouring row": [], "zeroed channel": []}
    for j, t in _probes(case):
        rows = np.array([j])
        drop = d["nbr"].copy()
        drop[j, t] = -1
        margins["dropped entry"].append(float((np.abs(_rows_ref(case, rows, nbr=drop) - ref[rows]) / tol[rows]).max()))
        if case.n_in > 1:
            move = d["nbr"].copy()
            move[j, t] = move[j, t] + 1 if move[j, t] + 1 < case.n_in else move[j, t] - 1
            margins["neighbouring row"].append(float((np.abs(_rows_ref(case, rows, nbr=move) - ref[rows]) / tol[rows]).max()))
        f = d["feats"].copy()
        f[:, (j + t) % case.c0] = 0.0
        margins["zeroed channel"].append(float((np.abs(_rows_ref(case, rows, feats=f) - ref[rows]) / tol[rows]).max()))
    for what, m in margins.items():
        assert m, what
        print(f"{case.name}: {what}: smallest max|delta|/tol over {len(m)} probes = {min(m):.1f}")
        assert min(m) > 8.0, (what, min(m))


def test_special_rows_are_in_the_tables():
    for case in (SC.LARGEST, SC.SPLIT_CASES[6], SC.DMA64_CASES[2]):
        nbr = SC.inputs(case)["nbr"]
        empty, same, pin = SC.special_rows(case.n_out)
        assert empty and (nbr[empty] == -1).all()
        assert all(len(set(nbr[r].tolist())) == 1 and nbr[r, 0] >= 0 for r in same)
        assert all(nbr[r, 0] == 0 and nbr[r, -1] == case.n_in - 1 for r in pin)
        assert nbr.min() == -1 and nbr.max() == case.n_in - 1 and 0.25 < (nbr < 0).mean() < 0.45


def test_every_kernel_form_has_a_case_with_empty_rows():
    small = [c for c in SC.PLAIN_CASES if c.n_out <= 1000]
    for kernel, narrow in ((SC.SPLITK, True), (SC.SPLITK, False), (SC.DMA64, True), (SC.DMA64, False)):
        assert any((SC.inputs(c)["nbr"] < 0).all(1).sum() >= 2 for c in small if SC.KERNEL_OF[c] == kernel and (c.cout <= 32) == narrow)
    for c in SC.COLLAPSED_CASES + SC.DMA64_CASES[6:] + SC.DMA64X128_CASES + SC.DMA128_CASES:      # special_rows: every table of 8 rows or more
        assert c.n_out >= 8 and c.table == "plain"
    assert {SC.KERNEL_OF[c] for c in SC.PLAIN_CASES} == {SC.SPLITK, SC.DMA64, SC.DMA64X128, SC.DMA128}


def test_group_live_sets_have_the_patterns_the_mask_walk_must_survive():
    live = SC.group_live_sets("hashed", 83237, 27)
    assert live.shape == (1301, 27)
    n = live.sum(1)
    assert (~live[:, 0] & live[:, 1:].all(1)).any() and (~live[:, 26] & live[:, :26].all(1)).any()      # lacks the first / the last tap only
    assert (n == 1).any() and (n == 0).any() and (n == 27).any()
    assert (live[n == 1][:, 0]).any() and (live[n == 1][:, 26]).any()                                   # the single tap is the first / the last
    runs = [r for r in live if 2 <= (~r).sum() < 27 and np.ptp(np.nonzero(~r)[0]) + 1 == (~r).sum()]
    assert runs                                                                                         # a run of consecutive dead taps
    par = SC.group_live_sets("parity", 131109, 27)
    assert not (par[0::2][:1024] & par[1::2][:1024]).any() and (par[0] | par[1]).all()
    rot = SC.group_live_sets("rotate", 200, 3)
    assert rot.tolist() == [[False, True, True], [True, True, False], [True, False, True], [False, True, True]]
    # the table really has those groups: the true liveness per 64 rows (what SparseEncoder._tile_mask computes) is inside the live set
    for case, _ in SC.MASK_CASES[:2]:
        nbr = SC.inputs(case)["nbr"]
        lv = SC.group_live_sets(case.table, case.n_out, case.ntaps)
        pad = (-case.n_out) % 64
        got = np.concatenate([nbr >= 0, np.zeros((pad, case.ntaps), bool)]).reshape(-1, 64, case.ntaps).any(1)
        assert not (got & ~lv).any() and (got == lv)[:-1].all()


def test_reference_agrees_with_the_encoder_oracle_on_a_real_table():
    """The synthetic tables mean what the encoder's tables mean: on the submanifold table of real coordinates the float64 reference
    equals oracle.sparse_encoder_ref.conv_features (fp32, taps in order) within the fp32 bound."""
    tag = "grid32x24x27"
    _, c, _ = cases.sparse_inputs(tag)
    shape = cases.sparse_cfg(tag)["sparse_shape"]
    coords = c.numpy()
    tab = SR.neighbour_table(coords, shape, coords, [3, 3, 3], [1, 1, 1], [0, 0, 0], True)
    assert (tab >= 0).sum() > 2 * tab.shape[0] and (tab < 0).any()      # neighbourhoods are populated, and not full
    n, c0, cout = coords.shape[0], 16, 32
    feats = hashfill.normal("sc_oracle_x", (n, c0), 1).numpy()
    w = hashfill.uniform("sc_oracle_w", (3, 3, 3, c0, cout), -1, 1, 3).numpy() * np.float32((3.0 / (c0 * 27)) ** 0.5)
    want = SR.conv_features(feats, tab, w)
    one, zero = np.ones(cout, np.float32), np.zeros(cout, np.float32)
    ref = SC.reference(feats, tab, w.reshape(27, c0, cout), one, zero, "none", None, False)
    tol = SC.bound(feats, tab, w.reshape(27, c0, cout), one, zero, None)
    assert np.abs(ref).max() > 0.5 and (np.abs(want - ref) <= tol).all()
    # ... and the strided table of the same sites
    oc, _ = SR.down_sites(coords, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1])
    tab2 = SR.neighbour_table(coords, shape, oc, [3, 3, 3], [2, 2, 2], [1, 1, 1], False)
    want2 = SR.conv_features(feats, tab2, w)
    ref2 = SC.reference(feats, tab2, w.reshape(27, c0, cout), one, zero, "none", None, False)
    assert (np.abs(want2 - ref2) <= SC.bound(feats, tab2, w.reshape(27, c0, cout), one, zero, None)).all()
