"""The float64 k-means reference (tests/kmeans_ref.py) against a brute-force loop, against scikit-learn's Lloyd iteration, and
against planted errors: a reference that breaks ties upward or divides by the wrong count must be caught.  Also the two claims
the GPU tests lean on: the band covers an fp32 accumulation in any order, and on the seeded Gaussian inputs the reference alone
leaves few rows undecided."""
import numpy as np
import pytest
import torch

from tests import kmeans_ref as R


def _grid(N, K, d, levels, seed):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randint(-levels, levels + 1, (N, d), generator=g).float() / levels).to(torch.bfloat16)
    C = (torch.randint(-levels, levels + 1, (K, d), generator=g).float() / levels).to(torch.bfloat16)
    return X, C


def _brute_assign(X, C, hn):
    x, c = X.double().numpy(), C.double().numpy()
    labels, best, second = [], [], []
    for i in range(x.shape[0]):
        vals = [float(np.dot(x[i], c[k])) - (0.0 if hn is None else float(hn[k])) for k in range(c.shape[0])]
        top = max(vals)
        lab = vals.index(top)                         # the first (lowest) id that attains it
        labels.append(lab)
        best.append(top)
        second.append(max(vals[:lab] + vals[lab + 1:], default=-float("inf")))
    return labels, best, second


def test_assignment_equals_brute_force_with_ties_to_the_lower_id():
    tied = 0
    for seed, (N, K) in enumerate([(40, 1), (40, 2), (200, 23), (200, 90)]):
        X, C = _grid(N, K, 64, 2, seed)
        for hn in (None, 0.5 * C.double().square().sum(1)):
            V = R.values64(X, C, hn)
            labels, best, second = R.assign64(V)
            bl, bb, bs = _brute_assign(X, C, hn)
            assert labels.tolist() == bl and best.tolist() == bb and second.tolist() == bs
            tied += int(R.tied_rows(V).sum())
            if K > 1:
                run = R.runner_up(V, labels)
                assert bool((run != labels).all()) and torch.equal(V[torch.arange(N), run], second)
    assert tied > 10                                   # the inputs do exercise the tie rule


def test_one_iteration_equals_scikit_learn():
    from sklearn.cluster import KMeans

    g = torch.Generator().manual_seed(0)
    N, K, d = 500, 7, 64
    X = (torch.randn(N, d, generator=g) + 3.0 * torch.randn(K, d, generator=g)[torch.arange(N) % K]).to(torch.bfloat16)
    C0 = X[torch.randperm(N, generator=g)[:K]].double()       # points as centroids: no cluster starts empty
    labels, _, _ = R.assign64(R.values64(X, C0, 0.5 * C0.square().sum(1)))
    counts, cent = R.update64(X, labels, C0)
    assert int(counts.min()) > 0
    sk = KMeans(n_clusters=K, init=C0.numpy(), n_init=1, max_iter=1, algorithm="lloyd", tol=0.0).fit(X.double().numpy())
    assert np.allclose(sk.cluster_centers_, cent.numpy(), rtol=0, atol=1e-9)
    # scikit-learn's labels_ are the assignment to the centres it returns
    relabel, best, _ = R.assign64(R.values64(X, cent, 0.5 * cent.square().sum(1)))
    assert sk.labels_.tolist() == relabel.tolist()
    inertia = float((X.double().square().sum(1) - 2.0 * best).sum())   # sum |x|^2 - 2 best, the objective KMeans reports
    assert abs(inertia - sk.inertia_) <= 1e-9 * sk.inertia_
    # lloyd_step64 is those pieces put together (centroids seen in bf16, as the kernel sees them)
    l2, _, c2, cent2 = R.lloyd_step64(X, C0.float())
    assert torch.equal(l2, labels) and torch.equal(c2, counts) and torch.equal(cent2, cent)
    # planted: a wrong divisor moves every centroid far outside the agreement above
    _, wrong = R.update64(X, labels, C0, count_offset=1)
    assert not np.allclose(sk.cluster_centers_, wrong.numpy(), rtol=0, atol=1e-6)


def test_planted_tie_break_is_caught():
    X, C = _grid(300, 200, 64, 2, 3)
    V = R.values64(X, C)
    assert int(R.tied_rows(V).sum()) > 5
    labels, best, second = R.assign64(V)
    up, best_up, second_up = R.assign64(V, ties="upper")
    bl, _, _ = _brute_assign(X, C, None)
    assert torch.equal(best, best_up) and torch.equal(second, second_up)     # the values cannot tell the two apart
    assert labels.tolist() == bl and up.tolist() != bl                         # the labels do
    assert bool((up[R.tied_rows(V)] > labels[R.tied_rows(V)]).all())


def test_spherical_update_and_empty_clusters():
    X, _ = R.gaussian_operands(50, 2, 64, unit=False, seed=4)
    labels = torch.arange(50) % 3                                              # clusters 3 and 4 of 5 stay empty
    prev = torch.randn(5, 64, generator=torch.Generator().manual_seed(1)).double()
    counts, cent = R.update64(X, labels, prev, spherical=True)
    assert counts.tolist() == [17, 17, 16, 0, 0]
    assert torch.allclose(cent[:3].norm(dim=1), torch.ones(3, dtype=torch.float64), rtol=0, atol=1e-14)
    s0 = X[labels == 0].double().sum(0)
    assert torch.allclose(cent[0], s0 / s0.norm(), rtol=0, atol=1e-14)
    assert torch.equal(cent[3:], prev[3:])
    _, mean = R.update64(X, labels, prev)
    assert torch.allclose(mean[1], X[labels == 1].double().mean(0), rtol=0, atol=1e-14) and torch.equal(mean[3:], prev[3:])


def test_reseed_rule():
    best = torch.tensor([0.5, -2.0, 0.25, -2.0, 3.0, -1.0])
    counts = torch.tensor([2, 0, 3, 0, 0, 1])
    # ascending empty cluster ids 1, 3, 4 take the points in ascending (best, id): 1 (-2.0), 3 (-2.0, the higher id), 5 (-1.0)
    assert R.reseed_points(best, counts) == {1: 1, 3: 3, 4: 5}
    assert R.reseed_points(best, torch.tensor([1, 1])) == {}
    # more empty clusters than points: the first ones are served
    assert R.reseed_points(torch.tensor([1.0, 0.0]), torch.tensor([0, 0, 0])) == {0: 1, 1: 0}
    # in a whole step: a centroid far from everything comes out empty and lands on the point with the smallest best
    X, _ = R.gaussian_operands(40, 2, 64, unit=False, seed=9)
    C = torch.cat([X[:2].float(), torch.full((1, 64), 100.0)])
    labels, b, counts, cent = R.lloyd_step64(X, C)
    assert counts[2] == 0 and int(labels.max()) == 1
    assert torch.equal(cent[2], X[int(torch.argmin(b))].double())


def test_half_norm_definition():
    _, C = R.gaussian_operands(1, 37, 320, unit=False, seed=2)
    h = R.half_norm32(C)
    assert h.dtype == torch.float32
    assert torch.allclose(h.double(), 0.5 * C.double().square().sum(1), rtol=320 * 2.0 ** -24, atol=0)
    _, G = _grid(1, 9, 64, 8, 0)                                                # exact in fp32: equal to float64
    assert torch.equal(R.half_norm32(G).double(), 0.5 * G.double().square().sum(1))


def test_band_bounds_fp32_values_in_any_order():
    X, C = R.gaussian_operands(16, 40, 320, unit=False, seed=3)
    hn = R.half_norm32(C)
    V = R.values64(X, C, hn)
    labels, best, second = R.assign64(V)
    B = R.band(X, C, labels, R.runner_up(V, labels), hn)
    prod = X.float()[:, None, :] * C.float()[None, :, :]                        # exact in fp32
    fwd, rev = torch.zeros(16, 40), torch.zeros(16, 40)
    for i in range(320):
        fwd = fwd + prod[:, :, i]
        rev = rev + prod[:, :, 319 - i]
    pair = prod.reshape(16, 40, 10, 32).sum(3).sum(2)
    rows = torch.arange(16)
    for acc in (fwd, rev, pair):
        got = acc - hn[None, :]                                                 # one fp32 subtraction
        assert bool(((got[rows, labels].double() - best).abs() <= B).all())
    assert float((B / best.abs().clamp_min(1.0)).max()) < 1e-4                  # and it is narrow


@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("N,K,d", R.RANDOM_SHAPES)
def test_reference_leaves_few_rows_undecided(N, K, d, unit):
    """The condition of the GPU test on random data, for the reference alone: at most 2 % of the rows have a float64 gap
    between best and second inside the band (measured here: at most 0.8 %)."""
    X, C = R.gaussian_operands(N, K, d, unit)
    for hn in (None, R.half_norm32(C)):
        V = R.values64(X, C, hn)
        labels, best, second = R.assign64(V)
        undecided = (best - second) <= R.band(X, C, labels, R.runner_up(V, labels), hn)
        print(f"N={N} K={K} d={d} unit={unit} bias={hn is not None}: {int(undecided.sum())} of {N} undecided")
        assert int(undecided.sum()) <= 0.02 * N
