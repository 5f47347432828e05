"""GPU checks of k-means (csrc/kmeans.hip through the C ABI and contrastors_amd.cluster.KMeans) against the float64 reference
of tests/kmeans_ref.py: the assignment bit for bit on operands whose fp32 arithmetic is exact (tile edges, ties, with and without
the bias), equal to the search kernel's bits, and inside a derived band on random data; the update per element against the fp32
running-sum bound, its shadow / half-norm / empty-cluster contract and run-to-run equality; KMeans end to end; the refusals."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS, KS, DS = [1, 127, 129, 300], [1, 2, 127, 129, 257, 1000], [64, 320, 1024]
EVAL_SEED = 34   # the first seed whose CPU draw of 8 rows of _blobs() holds one row of every blob (8! / 8^8 of them do)


def _grid_operands(N, K, d, levels, seed):
    """Entries from {-levels..levels}/levels (as tests/test_range_search_gpu.py): exact in bf16, products multiples of
    1/levels^2, |score| <= d <= 2^10 -- every partial sum is a multiple of 2^-6 below 2^11, and |c|^2 / 2 a multiple of 2^-7 below
    2^10: scores, half norms and their differences are exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    X = (torch.randint(-levels, levels + 1, (N, d), generator=g).float() / levels).to(torch.bfloat16)
    C = (torch.randint(-levels, levels + 1, (K, d), generator=g).float() / levels).to(torch.bfloat16)
    return X.to(DEV), C.to(DEV)


def _assign(X, C, hn, second=True):
    """cx_kmeans_assign on device operands -> (labels int32, best, second or None)."""
    from contrastors_amd import _C

    N, K, d = X.shape[0], C.shape[0], X.shape[1]
    labels = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    best = torch.full((N,), math.nan, dtype=torch.float32, device=DEV)
    sec = torch.full((N,), math.nan, dtype=torch.float32, device=DEV) if second else None
    _C.check(_C.lib().cx_kmeans_assign(X.data_ptr(), C.data_ptr(), _C.ptr(hn), N, K, d, X.stride(0), C.stride(0),
                                       labels.data_ptr(), best.data_ptr(), _C.ptr(sec), None), "cx_kmeans_assign")
    torch.cuda.synchronize()
    return labels, best, sec


def _check_exact(X, C, hn):
    V = R.values64(X, C, hn)
    want_l, want_b, want_s = R.assign64(V)
    labels, best, sec = _assign(X, C, hn)
    assert torch.equal(labels.long(), want_l), "labels differ from the reference"
    assert torch.equal(best.double(), want_b), "best differs from the reference"
    assert torch.equal(sec.double(), want_s), "second differs from the reference"
    return V


# ---- 1. exact operands: bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_assign_exact_grid(N, K, d):
    X, C = _grid_operands(N, K, d, 8, 1000 * N + K + d)
    _check_exact(X, C, None)
    _check_exact(X, C, R.half_norm32(C))


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_assign_exact_grid_ties(N, K, d):
    X, C = _grid_operands(N, K, d, 2, 1000 * N + K + d)
    V = _check_exact(X, C, None)
    Vb = _check_exact(X, C, R.half_norm32(C))
    if d == 64 and N >= 127 and K >= 127:   # the variant is here for its ties: maxima attained more than once
        assert int(R.tied_rows(V).sum()) >= 3 and int(R.tied_rows(Vb).sum()) >= 1


def test_assign_without_second_and_with_strides():
    X, C = _grid_operands(300, 257, 64, 8, 5)
    hn = R.half_norm32(C)
    want = _assign(X, C, hn)
    labels, best, sec = _assign(X, C, hn, second=False)
    assert sec is None and torch.equal(labels, want[0]) and torch.equal(best, want[1])
    Xw = torch.zeros(300, 128, dtype=torch.bfloat16, device=DEV)      # rows of a wider buffer: ldx = 128
    Xw[:, :64] = X
    got = _assign(Xw[:, :64], C, hn)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- 2. the search kernel's bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
def test_assign_equals_search(d):
    from contrastors_amd.search import FlatIPIndex

    X, C = R.gaussian_operands(1000, 1000, d, unit=True)
    X, C = X.to(DEV), C.to(DEV)
    ix = FlatIPIndex(d, device=DEV)
    ix.add(C)
    s, i = ix.search(X, 1)
    labels, best, _ = _assign(X, C, None)
    assert torch.equal(labels.long(), i[:, 0])
    assert torch.equal(best.view(torch.int32), s[:, 0].contiguous().view(torch.int32))


# ---- 3. random data against float64 with the derived band ------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("N,K,d", R.RANDOM_SHAPES)
def test_assign_random_within_band(N, K, d, unit):
    X, C = R.gaussian_operands(N, K, d, unit)
    X, C = X.to(DEV), C.to(DEV)
    for hn in (None, R.half_norm32(C)):
        V = R.values64(X, C, hn)
        want_l, want_b, want_s = R.assign64(V)
        B = R.band(X, C, want_l, R.runner_up(V, want_l), hn)
        decided = (want_b - want_s) > B
        labels, best, sec = _assign(X, C, hn)
        wrong = int((labels.long() != want_l)[decided].sum())
        eb, es = float(((best.double() - want_b).abs() / B).max()), float(((sec.double() - want_s).abs() / B).max())
        print(f"N={N} K={K} d={d} unit={unit} bias={hn is not None}: {int((~decided).sum())} undecided, {wrong} decided rows "
              f"mislabelled, |best - ref| <= {eb:.3f} band, |second - ref| <= {es:.3f} band")
        assert int((~decided).sum()) <= 0.02 * N
        assert wrong == 0
        assert eb <= 1.0 and es <= 1.0


# ---- 4. the update, per element -----------------------------------------------------------------------------------------------
def _update_labels(kind):
    g = torch.Generator().manual_seed(11)
    if kind == "edges":
        sizes = [0, 1, 255, 256, 257, 513]
    else:                                     # one cluster owns 90 % of 3000 points; cluster 0 is empty
        rest = torch.randint(2, 7, (300,), generator=g)
        sizes = [0, 2700] + torch.bincount(rest, minlength=7)[2:].tolist()
    labels = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return labels[torch.randperm(labels.numel(), generator=g)], sizes


def _update(X, labels, K, spherical, fill):
    """cx_kmeans_partial + cx_kmeans_finish over _update_plan; the outputs start from `fill` values."""
    from contrastors_amd import _C
    from contrastors_amd.cluster import _update_plan

    N, d = X.shape
    order, p_start, p_end, _, p_ptr, n_pieces = _update_plan(labels.to(DEV).to(torch.int32), K)
    mp = p_start.numel()
    partial = torch.full((mp, d), math.nan, dtype=torch.float32, device=DEV)
    counts = torch.full((K,), -7, dtype=torch.int32, device=DEV)
    cent = torch.full((K, d), fill, dtype=torch.float32, device=DEV)
    shadow = torch.full((K, d), fill, dtype=torch.bfloat16, device=DEV)
    hn = torch.full((K,), fill, dtype=torch.float32, device=DEV)
    h = _C.lib()
    _C.check(h.cx_kmeans_partial(X.data_ptr(), N, d, X.stride(0), order.data_ptr(), p_start.data_ptr(), p_end.data_ptr(),
                                 n_pieces.data_ptr(), mp, partial.data_ptr(), None), "cx_kmeans_partial")
    _C.check(h.cx_kmeans_finish(partial.data_ptr(), p_start.data_ptr(), p_end.data_ptr(), p_ptr.data_ptr(), K, d, mp,
                                int(spherical), counts.data_ptr(), cent.data_ptr(), shadow.data_ptr(), d, hn.data_ptr(), None),
             "cx_kmeans_finish")
    torch.cuda.synchronize()
    return counts, cent, shadow, hn


@pytest.mark.parametrize("spherical", [False, True])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind", ["edges", "skewed"])
def test_update_per_element(kind, d, spherical):
    """Bounds (no measurement behind them): a cluster's fp32 sum is count - 1 + pieces - 1 additions in some fixed tree, each
    off by at most 2^-24 of a partial sum that is at most A_j = sum_i |x_ij|, so |sum_j - exact| <= 2^-24 (count + pieces) A_j.
    Mean: divided by count, plus the division's rounding: within 2^-23 (count + pieces) A_j / count.  Unit-norm sum c = s / |s|:
    to first order |dc_j| <= (ds_j + |c_j| |ds|) / |s| plus the final rounding 2^-24 |c_j|: within
    2^-23 (count + pieces) (A_j + |c_j| |A|) / |s|; its norm within 2^-23 (count + pieces) of 1."""
    labels, sizes = _update_labels(kind)
    K, N = len(sizes), labels.numel()
    assert N == (1282 if kind == "edges" else 3000) and sizes[0] == 0 and (kind == "edges" or sizes[1] == 2700)
    X = (3.0 * torch.randn(N, d, generator=torch.Generator().manual_seed(d))).to(torch.bfloat16).to(DEV)
    counts, cent, shadow, hn = _update(X, labels, K, spherical, 7.0)
    assert counts.tolist() == sizes
    lab = labels.to(DEV)
    prev = torch.full((K, d), 7.0, dtype=torch.float64, device=DEV)
    _, want = R.update64(X, lab, prev, spherical)
    A = R.abs_sums64(X, lab, K)
    cnt = torch.tensor(sizes, dtype=torch.float64, device=DEV)
    terms = cnt + torch.ceil(cnt / 256)
    live = cnt > 0
    if spherical:
        snorm = torch.zeros(K, d, dtype=torch.float64, device=DEV).index_add_(0, lab, X.double()).norm(dim=1)
        bound = 2.0 ** -23 * terms[:, None] * (A + want.abs() * A.norm(dim=1, keepdim=True)) / snorm.clamp_min(1e-300)[:, None]
        assert bool(((cent.double().norm(dim=1) - 1.0).abs() <= 2.0 ** -23 * terms)[live].all())
    else:
        bound = 2.0 ** -23 * terms[:, None] * A / cnt.clamp_min(1)[:, None]
    err = (cent.double() - want).abs()
    print(f"{kind} d={d} spherical={spherical}: max error / bound = {float((err / bound.clamp_min(1e-300))[live].max()):.3f}")
    assert bool((err <= bound)[live].all())
    assert torch.equal(shadow[live].view(torch.int16), cent[live].to(torch.bfloat16).view(torch.int16))
    want_hn = torch.zeros(K, dtype=torch.float32, device=DEV) if spherical else R.half_norm32(shadow)
    assert torch.equal(hn[live].view(torch.int32), want_hn[live].view(torch.int32))
    # empty clusters: count 0, everything else as it was
    assert bool((cent[~live] == 7.0).all()) and bool((shadow[~live] == 7.0).all()) and bool((hn[~live] == 7.0).all())
    # a second run gives the same bits
    again = _update(X, labels, K, spherical, 7.0)
    for a, b in zip((counts, cent, shadow.view(torch.int16), hn), (again[0], again[1], again[2].view(torch.int16), again[3])):
        assert torch.equal(a, b)


# ---- 5. KMeans end to end ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blobs():
    """8 blobs of 200 points in 64 dimensions: centres ~ 10 * N(0, 1) per coordinate (about 110 apart), noise N(0, 1) (about 8
    from its centre); shuffled.  -> (points fp32 CPU, planted labels)."""
    g = torch.Generator().manual_seed(0)
    centres = 10.0 * torch.randn(8, 64, generator=g)
    y = torch.arange(1600)[torch.randperm(1600, generator=g)] % 8
    return centres[y] + torch.randn(1600, 64, generator=g), y


def test_kmeans_recovers_planted_blobs():
    from contrastors_amd.cluster import KMeans

    x, y = _blobs()
    init = torch.stack([x[int(torch.nonzero(y == c)[0])] for c in range(8)])       # one member per blob, in blob order
    for spherical in (False, True):
        km = KMeans(8, 64, spherical=spherical, device=DEV).fit(x, init=init)
        assert km.labels_.dtype == torch.int32 and torch.equal(km.labels_.cpu().long(), y)
        assert km.converged_ and 1 <= km.n_iter_ <= 3
        assert km.counts_.tolist() == [200] * 8
        assert km.centroids.dtype == torch.float32 and tuple(km.centroids.shape) == (8, 64)
        xb = x.to(torch.bfloat16).to(DEV)
        _, want = R.update64(xb, y.to(DEV), torch.zeros(8, 64, device=DEV), spherical)
        assert torch.allclose(km.centroids.double(), want, rtol=0, atol=1e-4)
        lab, best, _ = km.assign(xb)
        want_obj = float(best.double().sum()) if spherical else float(xb.double().square().sum() - 2.0 * best.double().sum())
        assert torch.equal(lab, km.labels_) and km.objective_ == pytest.approx(want_obj, rel=1e-12)
    assert km.objective_ > 0


def test_kmeans_reseeds_an_empty_cluster_by_the_rule():
    from contrastors_amd.cluster import KMeans

    x, y = _blobs()
    xb = x.to(torch.bfloat16)
    init = torch.cat([torch.stack([x[int(torch.nonzero(y == c)[0])] for c in range(8)]), torch.full((1, 64), 1000.0)])
    km = KMeans(9, 64, device=DEV)
    km.set_centroids(init)
    labels, best, counts = km.step(x)
    assert counts.tolist() == [200] * 8 + [0] and torch.equal(labels.cpu().long(), y)
    named = R.reseed_points(best.cpu(), counts.cpu())
    want = R.lloyd_step64(xb.to(DEV), init.to(DEV))
    assert list(named) == [8] and torch.equal(want[3][8].cpu(), xb[named[8]].double())   # the reference names the same point
    assert torch.equal(km.centroids[8].cpu(), xb[named[8]].float())
    assert torch.allclose(km.centroids[:8].double(), want[3][:8], rtol=0, atol=1e-4)
    # the re-seeded centroid is live in the next assignment: its own point goes to it
    lab2, _, _ = km.assign(xb.to(DEV))
    assert int(lab2[named[8]]) == 8


def test_kmeans_same_seed_same_bits():
    from contrastors_amd.cluster import KMeans

    x, _ = _blobs()
    runs = [KMeans(8, 64, device=DEV, seed=3).fit(x, n_init=2, max_iter=10) for _ in range(2)]
    assert torch.equal(runs[0].centroids.view(torch.int32), runs[1].centroids.view(torch.int32))
    assert torch.equal(runs[0].labels_, runs[1].labels_) and runs[0].objective_ == runs[1].objective_
    assert runs[0].n_iter_ == runs[1].n_iter_ >= 1
    sub = [KMeans(8, 64, spherical=True, device=DEV, seed=5).fit(x, sample=500, max_iter=10) for _ in range(2)]
    assert torch.equal(sub[0].centroids.view(torch.int32), sub[1].centroids.view(torch.int32))
    assert torch.equal(sub[0].labels_, sub[1].labels_) and sub[0].labels_.numel() == 1600


def test_kmeans_assign_streams_a_host_memmap(tmp_path):
    from contrastors_amd.cluster import KMeans

    x, y = _blobs()
    km = KMeans(8, 64, device=DEV)
    km.set_centroids(torch.stack([x[int(torch.nonzero(y == c)[0])] for c in range(8)]))
    want = km.assign(x.to(torch.bfloat16).to(DEV))
    np.save(tmp_path / "x.npy", x.numpy())
    mm = np.load(tmp_path / "x.npy", mmap_mode="r")
    got = km.assign(mm, batch_rows=333)                                               # 1600 = 4 * 333 + 268
    assert all(isinstance(g, np.ndarray) for g in got) and got[0].dtype == np.int32
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    host = km.assign(x, batch_rows=1000)                                              # a CPU tensor: torch out, on the device
    assert all(torch.equal(a, b) for a, b in zip(host, want))


def test_evaluate_clustering_on_blobs():
    """k-means from random rows separates 8 far blobs only if the draw holds one row of each (a Lloyd step cannot move a centroid
    across blobs), so the seed is one whose draw does; the test checks that first."""
    from contrastors_amd.cluster import evaluate_clustering

    x, y = _blobs()
    seed = EVAL_SEED
    draw = torch.randperm(1600, generator=torch.Generator().manual_seed(seed))[:8]
    assert sorted(y[draw].tolist()) == list(range(8))
    names = np.array(list("abcdefgh"))[y.numpy()]
    for spherical in (True, False):
        out = evaluate_clustering(x, names, spherical=spherical, seed=seed, n_init=1, device=DEV)
        assert set(out) == {"v_measure", "homogeneity", "completeness", "k", "n"}
        assert out["k"] == 8 and out["n"] == 1600
        assert out["v_measure"] == pytest.approx(1.0, abs=1e-12) and out["homogeneity"] == pytest.approx(1.0, abs=1e-12)



def test_tool_end_to_end(tmp_path, capsys):
    import json

    from contrastors_amd.tools import cluster as tool

    x, y = _blobs()
    np.save(tmp_path / "x.npy", x.numpy())
    np.save(tmp_path / "y.npy", y.numpy())
    base = ["--embeddings", str(tmp_path / "x.npy"), "--k", "8", "--device", DEV]
    assert tool.main(base + ["--out", str(tmp_path / "l.npy"), "--centroids_out", str(tmp_path / "c.npy"), "--seed",
                             str(EVAL_SEED), "--labels", str(tmp_path / "y.npy")]) == 0
    report, evaluation = (json.loads(line) for line in capsys.readouterr().out.strip().splitlines())
    labels, cent = np.load(tmp_path / "l.npy"), np.load(tmp_path / "c.npy")
    assert labels.dtype == np.int32 and labels.shape == (1600,) and cent.dtype == np.float32 and cent.shape == (8, 64)
    assert report["n"] == 1600 and report["k"] == 8 and report["converged"] and report["n_iter"] >= 1
    assert evaluation["v_measure"] == pytest.approx(1.0, abs=1e-12) and evaluation["k"] == 8 and evaluation["n"] == 1600
    for c in range(8):                                      # every centroid is the mean of its blob
        assert np.allclose(cent[c], x[torch.from_numpy(labels == c)].to(torch.bfloat16).double().mean(0).numpy(), rtol=0, atol=1e-4)
    # fitted on a subsample, spherical: every row is still labelled, and a second run writes the same bytes
    for name in ("s1.npy", "s2.npy"):
        assert tool.main(base + ["--out", str(tmp_path / name), "--spherical", "--sample", "800", "--n_init", "2"]) == 0
    s1, s2 = np.load(tmp_path / "s1.npy"), np.load(tmp_path / "s2.npy")
    assert s1.shape == (1600,) and 0 <= int(s1.min()) and int(s1.max()) < 8 and s1.tolist() == s2.tolist()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from contrastors_amd import _C

    h = _C.lib()
    X, C = _grid_operands(129, 257, 64, 8, 1)
    X96, C96 = torch.zeros(129, 96, dtype=torch.bfloat16, device=DEV), torch.zeros(257, 96, dtype=torch.bfloat16, device=DEV)
    labels = torch.full((129,), -7, dtype=torch.int32, device=DEV)
    best = torch.full((129,), 5.0, dtype=torch.float32, device=DEV)
    sec = torch.full((129,), 5.0, dtype=torch.float32, device=DEV)

    def rc(**kw):
        a = dict(X=X.data_ptr(), C=C.data_ptr(), hn=None, N=129, K=257, d=64, ldx=64, ldc=64, label=labels.data_ptr(),
                 best=best.data_ptr(), second=sec.data_ptr())
        a.update(kw)
        return h.cx_kmeans_assign(*a.values(), None)

    assert rc(d=96, ldx=96, ldc=96, X=X96.data_ptr(), C=C96.data_ptr()) == -1                    # CX_ERR_SHAPE
    assert rc(K=0) == -1 and rc(d=2048, ldx=2048, ldc=2048) == -1 and rc(N=-1) == -1 and rc(N=2 ** 31 - 128) == -1
    assert rc(label=None) == -3 and rc(best=None) == -3 and rc(X=None) == -3 and rc(C=None) == -3   # CX_ERR_ARG
    assert rc(ldx=60) == -2 and rc(ldc=68) == -2 and rc(X=X.data_ptr() + 2) == -2                  # CX_ERR_ALIGN
    assert rc(N=0, X=None, label=None, best=None) == 0
    torch.cuda.synchronize()
    assert bool((labels == -7).all()) and bool((best == 5.0).all()) and bool((sec == 5.0).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool((labels >= 0).all())
    # the update's entry points
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    order, ps, pe, pp, npc = i32(*range(129)), i32(0, 0), i32(129, 0), i32(0, 1), i32(1)
    partial = torch.full((2, 64), 3.0, dtype=torch.float32, device=DEV)
    counts, cent = i32(-7), torch.full((1, 64), 3.0, dtype=torch.float32, device=DEV)
    shadow, hn = torch.full((1, 64), 3.0, dtype=torch.bfloat16, device=DEV), torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
    part = lambda **kw: h.cx_kmeans_partial(*{**dict(X=X.data_ptr(), N=129, d=64, ldx=64, order=order.data_ptr(),
                                                     ps=ps.data_ptr(), pe=pe.data_ptr(), npc=npc.data_ptr(), mp=2,
                                                     partial=partial.data_ptr()), **kw}.values(), None)
    fin = lambda **kw: h.cx_kmeans_finish(*{**dict(partial=partial.data_ptr(), ps=ps.data_ptr(), pe=pe.data_ptr(),
                                                   pp=pp.data_ptr(), K=1, d=64, mp=2, sph=0, counts=counts.data_ptr(),
                                                   cent=cent.data_ptr(), shadow=shadow.data_ptr(), lds=64, hn=hn.data_ptr()),
                                              **kw}.values(), None)
    assert part(d=96) == -1 and part(N=-1) == -1 and part(order=None) == -3 and part(partial=None) == -3 and part(ldx=60) == -2
    assert fin(d=96) == -1 and fin(K=-1) == -1 and fin(counts=None) == -3 and fin(hn=None) == -3 and fin(lds=32) == -2
    assert part(N=0) == 0 and fin(K=0) == 0
    torch.cuda.synchronize()
    assert bool((partial == 3.0).all()) and int(counts) == -7 and bool((cent == 3.0).all()) and bool((hn == 3.0).all())
    assert part() == 0 and fin() == 0
    torch.cuda.synchronize()
    assert int(counts) == 129 and torch.allclose(cent[0].double(), X.double().mean(0), rtol=0, atol=1e-5)
    assert bool((partial[1] == 3.0).all())                                             # the piece past n_pieces was not written
