"""The col2im reference of tests/conv_backward_ref.py judged on its own, on the CPU: F.fold and the index
arithmetic agree on every case of the geometry table, the table tells every per-axis swap from the truth, and fold is
the adjoint of unfold."""
import pytest
import torch

import conv_backward_ref as B
import conv_geometry_ref as G


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_fold_and_gather_agree(case):
    P = B.make_rows(case, seed=G.CASE_IDS.index(case.id), integer=True, dtype=torch.float64)
    ref = B.fold_ref(P, case)
    assert ref.shape == case.xshape
    assert torch.equal(B.fold_gather(P, case), ref)          # integers: float64 sums are exact in any order
    counts = B.tap_counts(case)
    assert torch.equal(B.fold_ref(torch.ones_like(P), case), counts.double())
    assert int(counts.max()) <= case.k[0] * case.k[1]


def test_unread_elements_are_in_the_table():
    """Elements without a tap, which the kernel has to leave exactly 0: F4 (four trailing columns), A6 (1 x 1 at
    strides 2 and 3), G6 (dilated columns), A1 among others. (A5, whose padding passes the kernel's reach, has whole
    ROWS OF P on the padding instead; every image element of it is read.)"""
    by_id = dict(zip(G.CASE_IDS, G.CASES))
    unread = {c.id: int((B.tap_counts(c) == 0).sum()) for c in G.CASES}
    assert {cid for cid, n in unread.items() if n} == {"F2", "F3", "F4", "G1", "G2", "G5", "G6", "A1", "A6"}
    assert unread["F4"] == 2 * 3 * 32 * 4 and unread["A5"] == 0
    assert bool((B.tap_counts(by_id["F4"])[..., 48:] == 0).all())
    for c in G.CASES:
        assert bool((B.tap_counts(c) > 0).any()), c.id


@pytest.mark.parametrize("mutation", B.MUTATIONS)
def test_every_swap_changes_a_case(mutation):
    changed = []
    for i, case in enumerate(G.CASES):
        P = B.make_rows(case, seed=50 + i, integer=True, dtype=torch.float64)
        if not torch.equal(B.fold_gather(P, case, mutation), B.fold_ref(P, case)):
            changed.append(case.id)
    print(f"{mutation}: changes {changed}")
    assert changed, mutation


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_fold_is_the_adjoint_of_unfold(case):
    """<fold(P), X> == <P, unfold(X)> on integers in float64 (both sides exact)."""
    gen = torch.Generator().manual_seed(7 + G.CASE_IDS.index(case.id))
    X = torch.randint(-50, 51, case.xshape, generator=gen, dtype=torch.int64).double()
    P = B.make_rows(case, seed=90 + G.CASE_IDS.index(case.id), integer=True, dtype=torch.float64)
    lhs = (B.fold_ref(P, case) * X).sum()
    rhs = (P * G.unfold_rows(X, case)).sum()
    assert float(lhs) == float(rhs)
    assert float((B.fold_gather(P, case) * X).sum()) == float(rhs)
