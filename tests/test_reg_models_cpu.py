"""CPU tier, numpy alone: the conditions the matrices of tests/support/reg_models.py must meet for
tests/test_ldlt_batch_regularization_gpu.py to have ONE right answer per instance — conditions of the inputs, not
measurements of the product.

Every decision of the regularization ladder is an inertia count.  It must be far from turning at every rung any
compute() of the GPU tests tries (first from an empty memory, second from the first one's memory, third on ANOTHER
class with that memory), the unregularized attempt's |D| >= 1e-4 rule must not depend on the elimination order, and the
batch must really end on different rungs."""
import numpy as np
import pytest

from tests.support import reg_models as rm

EPS = float(np.finfo(np.float64).eps)
SHAPES = sorted(rm.SHAPES)


def _ladders(shape):
    """(class, label, expected) of every compute() the GPU tests make on this shape."""
    first = [rm.expected_of(shape, c) for c in range(rm.N_CLASSES)]
    second = [rm.expected_of(shape, c, first[c]["memory"][0]) for c in range(rm.N_CLASSES)]
    out = [(c, "first", first[c]) for c in range(rm.N_CLASSES)] + [(c, "second", second[c]) for c in range(rm.N_CLASSES)]
    for c in range(rm.N_CLASSES):
        for c_mem in range(rm.N_CLASSES):  # any class meeting any other's memory: every rotation of every batch
            out.append((c, f"after class {c_mem}", rm.expected_of(shape, c, second[c_mem]["memory"][0])))
    return out


def _ldlt_natural_order(K):
    """D of K = L D L^T without pivoting, columns in their natural order."""
    A = np.array(K, dtype=np.float64)
    dim = len(A)
    D = np.zeros(dim)
    for j in range(dim):
        D[j] = A[j, j]
        col = A[j + 1:, j] / D[j]
        A[j + 1:, j + 1:] -= np.outer(col, A[j + 1:, j])
    return D


@pytest.mark.parametrize("shape", SHAPES)
def test_matrices_are_finite_on_one_pattern_and_same_class_means_same_bits(shape):
    m = rm.model(shape)
    again = rm.classes(*rm.SHAPES[shape][:2], rm.SEED, rm.SHAPES[shape][2])
    assert m.vals.shape[0] == rm.N_CLASSES and np.isfinite(m.vals).all()
    assert np.array_equal(m.vals.view(np.uint64), again.vals.view(np.uint64))
    cols = np.repeat(np.arange(m.dim), np.diff(m.colptr))
    assert (m.rowidx >= cols).all()  # a lower triangle
    for c, K in enumerate(m.K):
        assert np.array_equal(K, K.T)
        back = np.zeros_like(K)
        back[m.rowidx, cols] = m.vals[c]
        assert np.array_equal(np.tril(K), back), c  # the pattern holds every entry of every class
    # class 7: a variable no row of A touches, cut loose in this class only
    assert not m.A[:, m.k].any()
    K7 = m.K[rm.GIVE_UP_CLASS]
    assert K7[m.k, m.k] == rm.CUT_LOOSE and np.count_nonzero(K7[m.k]) == 1
    assert np.count_nonzero(m.K[0][m.k]) > 1
    # the base: lambda_min(H0) >= 1, A of full row rank
    assert np.linalg.eigvalsh(m.H0)[0] >= 1.0
    assert np.linalg.matrix_rank(m.A) == m.m_e


@pytest.mark.parametrize("shape", SHAPES)
def test_every_rung_tried_is_far_from_a_change_of_inertia(shape):
    m = rm.model(shape)
    n, m_e = m.n, m.m_e
    worst_direct, worst_schur = np.inf, np.inf
    for c, label, e in _ladders(shape):
        K = m.K[c]
        k_inf = float(np.abs(K).sum(axis=1).max())
        for (delta, gamma), margin in zip(e["attempts"], e["margins"]):
            # the count expected() decided on: eigvalsh of the Schur complement, a thousand times eigvalsh's own
            # error (n eps |S|) away from a zero eigenvalue
            assert margin >= 1e3 * n * EPS, (c, label, delta, margin)
            worst_schur = min(worst_schur, margin)
            if delta > 1e3:
                # (class 7's ladder, and a class that meets class 7's memory: beside such a delta one eigvalsh of the
                # whole matrix returns the m_e eigenvalues near -1e-2 with an error of eps delta — the Schur complement
                # above is the count that stays exact)
                continue
            if c != rm.GIVE_UP_CLASS:
                # the condition as one eigvalsh of K + diag(delta, -gamma) states it: min |eig| >= 1e-9 |K|_inf — and
                # the same count
                counts, smallest = rm.direct_inertia(rm.regularized(K, n, delta, gamma))
                assert smallest >= rm.MARGIN * k_inf, (c, label, delta, smallest, k_inf)
                assert counts == rm.inertia(K, n, delta, gamma)[0], (c, label, delta)
                worst_direct = min(worst_direct, smallest / k_inf)
            else:
                # class 7 is the direct sum of the variable cut loose and the rest: the same condition block by block
                # (one eigvalsh of the whole would return the eigenvalues of order one with an error of eps 1e21)
                w, block_margin = rm.spectrum(rm.regularized(K, n, delta, gamma))
                assert block_margin >= rm.MARGIN, (label, delta, block_margin)
                assert (int((w > 0).sum()), int((w < 0).sum()), int((w == 0).sum())) == rm.inertia(K, n, delta, gamma)[0]
    print(f"{shape}: smallest |eig| / |K|_inf over every rung of classes 0-6 {worst_direct:.2e}; of the Schur complements "
          f"(over their own norm) {worst_schur:.2e}")
    assert worst_direct >= rm.MARGIN


@pytest.mark.parametrize("shape", SHAPES)
def test_unregularized_attempt_does_not_turn_on_the_elimination_order(shape):
    """Class 0 is quasi-definite with min(lambda_min(H), lambda_min(C)) >= 1e-4: whatever symmetric order a
    factorization takes, every |pivot| is at least that (the pivots of a positive definite matrix are bounded below by
    its smallest eigenvalue, and so are those of every Schur complement of a quasi-definite one)."""
    m = rm.model(shape)
    floor = min(float(np.linalg.eigvalsh(m.H0)[0]), rm.C22)
    assert floor >= 1e-4
    rng = np.random.default_rng(1)
    for _ in range(4):
        p = rng.permutation(m.dim)
        D = _ldlt_natural_order(m.K[0][np.ix_(p, p)])
        assert np.abs(D).min() >= floor * (1.0 - 1e-12)
        assert (D > 0).sum() == m.n and (D < 0).sum() == m.m_e


@pytest.mark.parametrize("shape", SHAPES)
def test_batches_end_on_different_rungs(shape):
    first = [rm.expected_of(shape, c) for c in range(rm.N_CLASSES)]
    accepted = {e["accepted"] for e in first if e["info"] == 0}
    assert len(accepted) >= 6, accepted
    assert [e["info"] for e in first] == [0] * 7 + [1]
    assert first[0]["accepted"] == (0.0, 0.0) and len(first[0]["attempts"]) == 1
    assert [e["accepted"][0] for e in first[1:7]] == [1e-4, 1e-4, 1e-3, 1e-1, 1.0, 100.0]
    # the give-up: the unregularized attempt, then delta = 1e-4 ... 1e20 (25 rungs; 1e21 is the first above the limit)
    give_up = first[rm.GIVE_UP_CLASS]
    assert give_up["accepted"] is None and len(give_up["attempts"]) == 26 and give_up["memory"][0] > 1e20
    assert np.isfinite(give_up["memory"]).all()
    # the second compute() separates the two classes of the lowest decade: prev / 2 = 5e-5 lies between their t
    second = [rm.expected_of(shape, c, first[c]["memory"][0]) for c in range(rm.N_CLASSES)]
    assert second[1]["accepted"] == (5e-5, 1e-10) and second[2]["accepted"] == (5e-4, 1e-10)
    assert len(second[rm.GIVE_UP_CLASS]["attempts"]) == 2 and second[rm.GIVE_UP_CLASS]["info"] == 1
    print(f"{shape}: first computes {[e['accepted'] for e in first]}; second {[e['accepted'] for e in second]}")


@pytest.mark.parametrize("shape", SHAPES)
def test_a_factorization_without_pivoting_counts_the_same_inertia(shape):
    """What makes the eigenvalue count the right reference for kernels that count the signs of D: for every matrix of
    every first and second ladder, D of an LDL^T without pivoting (here in the natural order) exists, is finite and has
    the inertia expected() decided on (Sylvester)."""
    m = rm.model(shape)
    for c in range(rm.N_CLASSES):
        e1 = rm.expected_of(shape, c)
        for e in (e1, rm.expected_of(shape, c, e1["memory"][0])):
            for delta, gamma in e["attempts"]:
                D = _ldlt_natural_order(rm.regularized(m.K[c], m.n, delta, gamma))
                assert np.isfinite(D).all() and (D != 0.0).all()
                counts = rm.inertia(m.K[c], m.n, delta, gamma)[0]
                assert (int((D > 0).sum()), int((D < 0).sum()), 0) == counts, (c, delta)


def test_batch_layouts():
    small = rm.batch_classes(5)
    assert small[2] == rm.GIVE_UP_CLASS and rm.GIVE_UP_CLASS not in np.delete(small, 2)
    assert len(set(small)) == 5  # accepted instances of different rungs on both sides of the give-up
    big = rm.batch_classes(70)
    assert np.array_equal(np.sort(big), np.sort(np.arange(70) % rm.N_CLASSES))
    assert len({big[63], big[64], big[69]}) == 3  # the last lane of the first 64, the first and last of the 6 beyond
    assert np.array_equal(big, rm.batch_classes(70))


def test_expected_refuses_what_inertia_alone_cannot_decide():
    m = rm.model("small")
    K = m.K[0].copy()
    K[0, 0] = np.nan
    with pytest.raises(ValueError):
        rm.expected(K, m.n, m.m_e)
    weak = m.K[0].copy()
    weak[m.n:, m.n:] = -1e-5 * np.eye(m.m_e)  # ideal inertia, but pivots below the 1e-4 rule are possible
    with pytest.raises(ValueError):
        rm.expected(weak, m.n, m.m_e)
