"""The numpy reference of the int8 scalar-quantised search (tests/int8_ref.py) against brute-force Python loops on tiny inputs,
against planted errors (each wrong variant of the loops must be told apart from the reference by at least one case here), and a
recall condition on the reference alone.  No GPU, no library call."""
import numpy as np
import pytest

from tests import int8_ref as R

F32 = np.float32


# ---- brute force: scalar loops, one fp32 operation per step; the keyword arguments plant the errors ---------------------
def _round_half_even(p):
    return float(round(float(p)))            # Python rounds exact halves to even


def _round_half_away(p):
    p = float(p)
    return float(np.floor(abs(p) + 0.5)) * (1.0 if p >= 0 else -1.0)


def loop_quantize(x, half_away=False, scale128=False, full_range=False, inv_from_scale=False):
    x = np.asarray(x, F32)
    codes = np.zeros(x.shape, np.int8)
    scales = np.zeros(x.shape[0], F32)
    for r, row in enumerate(x):
        amax = F32(0)
        for v in row:
            amax = max(amax, F32(abs(v)))
        if amax < F32(2.0 ** -100):
            continue
        scales[r] = F32(amax / F32(128 if scale128 else 127))
        inv = F32(F32(128 if full_range else 127) / amax)
        if inv_from_scale:
            inv = F32(F32(1) / scales[r])
        for j, v in enumerate(row):
            p = F32(F32(v) * inv)
            c = _round_half_away(p) if half_away else _round_half_even(p)
            codes[r, j] = int(min(max(c, -128.0 if full_range else -127.0), 127.0))
    return codes, scales


def loop_scores(qc, qs, dc, ds, swapped=False, fused=False):
    S = np.zeros((len(qc), len(dc)), F32)
    for m in range(len(qc)):
        for n in range(len(dc)):
            acc = sum(int(a) * int(b) for a, b in zip(qc[m], dc[n]))
            if fused:
                S[m, n] = F32(float(acc) * float(ds[n]) * float(qs[m]))       # float64 products, rounded once
            elif swapped:
                S[m, n] = F32(F32(F32(acc) * F32(qs[m])) * F32(ds[n]))
            else:
                S[m, n] = F32(F32(F32(acc) * F32(ds[n])) * F32(qs[m]))
    return S


def loop_topk(S, k, exclude=None, below=None, non_strict=False, ties_up=False, drop_exclusions=False):
    M, N = S.shape
    out_s = np.full((M, k), -np.inf, S.dtype)
    out_i = np.full((M, k), -1, np.int64)
    for m in range(M):
        ent = []
        for n in range(N):
            if below is not None and not (S[m, n] <= below[m] if non_strict else S[m, n] < below[m]):
                continue
            if exclude is not None and not drop_exclusions and n in exclude[m]:
                continue
            ent.append((-float(S[m, n]), -n if ties_up else n))
        ent.sort()
        for j, (s, n) in enumerate(ent[:k]):
            out_s[m, j], out_i[m, j] = S[m, abs(n)], abs(n)
    return out_s, out_i


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _half_rows():
    """amax = 127 * 2^e: inv is a power of two, so x = (k + 0.5) * 2^e lands exactly on k + 0.5, for even and odd k, both signs."""
    e = F32(2.0 ** -5)
    ks = np.array([0, 1, 2, 3, 64, 65, 125, 126, -1, -2, -3, -64, -125, -126], F32)
    row = np.zeros(64, F32)
    row[: ks.size] = (ks + np.sign(ks + F32(0.25)) * F32(0.5)) * e
    row[40] = F32(127) * e
    neg = row.copy()
    neg[40] = -neg[40]                        # the amax element negative
    return np.stack([row, neg])


def _inv_sensitive_row():
    """A row on which inv = 1 / scale rounds some element differently from inv = 127 / amax (found by a seeded scan)."""
    rng = np.random.default_rng(7)
    for amax in rng.uniform(0.5, 2.0, 400).astype(F32):
        inv_a, inv_b = F32(F32(127) / amax), F32(F32(1) / F32(amax / F32(127)))
        if inv_a == inv_b:
            continue
        for k in range(1, 126):
            x = F32(F32(k + 0.5) / inv_a)
            for _ in range(4):
                x = np.nextafter(x, F32(0))
            for _ in range(9):
                if abs(x) <= amax and np.rint(F32(x * inv_a)) != np.rint(F32(x * inv_b)):
                    row = np.zeros(64, F32)
                    row[0], row[1] = amax, x
                    return row[None, :]
                x = np.nextafter(x, F32(4))
    raise AssertionError("no sensitive row found")


def _rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(F32) * rng.uniform(0.01, 30, (n, 1)).astype(F32)
    return x


# ---- the quantiser -----------------------------------------------------------------------------------------------------
def test_quantize_equals_the_loops_on_random_edge_and_half_rows():
    x = _rows(6, 64, 1)
    x[1] = 0
    x[2] = F32(2.0 ** -101)                  # amax below 2^-100: a zero row
    x[3, :] = F32(2.0 ** -100)               # at the bound: quantised
    x[4, -1] = -100.0                        # the amax element is the last and negative
    for rows in (x, _half_rows(), _inv_sensitive_row()):
        got = R.quantize(rows)
        assert got[0].dtype == np.int8 and got[1].dtype == F32
        assert _same(got, loop_quantize(rows))
        assert got[0].min() >= -127
    c, s = R.quantize(x)
    assert not c[1].any() and s[1] == 0 and not c[2].any() and s[2] == 0
    assert s[3] == F32(F32(2.0 ** -100) / F32(127)) and (c[3] == 127).all()
    assert c[4, -1] == -127 and s[4] == F32(F32(100) / F32(127))
    h, _ = R.quantize(_half_rows())
    assert h[0, :8].tolist() == [0, 2, 2, 4, 64, 66, 126, 126] and h[0, 8:14].tolist() == [-2, -2, -4, -64, -126, -126]
    assert h[1, 40] == -127 and h[0, 40] == 127


@pytest.mark.parametrize("error, rows", [
    ("half_away", "half"), ("scale128", "random"), ("full_range", "half"), ("inv_from_scale", "sensitive")])
def test_planted_quantiser_errors_are_caught(error, rows):
    x = {"half": _half_rows(), "random": _rows(4, 64, 2), "sensitive": _inv_sensitive_row()}[rows]
    assert not _same(R.quantize(x), loop_quantize(x, **{error: True}))
    if error == "full_range":
        assert loop_quantize(x, full_range=True)[0].min() == -128 and R.quantize(x)[0].min() == -127


# ---- the score ---------------------------------------------------------------------------------------------------------
def _coded(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-127, 128, (n, d), dtype=np.int8), rng.uniform(1e-3, 3e-2, n).astype(F32)


def test_scores_equal_the_loops_and_saturate_exactly():
    qc, qs = _coded(5, 64, 3)
    dc, ds = _coded(9, 64, 4)
    S = R.scores(qc, qs, dc, ds)
    assert S.dtype == F32 and np.array_equal(S, loop_scores(qc, qs, dc, ds))
    sat = np.full((2, 1024), 127, np.int8)
    sat[1] = -127
    assert R.acc_matrix(sat, sat).tolist() == [[16516096, -16516096], [-16516096, 16516096]]
    one = np.ones(2, F32)
    assert R.scores(sat, one, sat, one).tolist() == [[16516096.0, -16516096.0], [-16516096.0, 16516096.0]]


@pytest.mark.parametrize("error", ["swapped", "fused"])
def test_planted_score_errors_are_caught(error):
    qc, qs = _coded(8, 64, 5)
    dc, ds = _coded(40, 64, 6)
    assert not np.array_equal(R.scores(qc, qs, dc, ds), loop_scores(qc, qs, dc, ds, **{error: True}))


# ---- top-k -------------------------------------------------------------------------------------------------------------
def _tied_scores():
    """5 rows x 12 documents with ties: documents n and n + 6 score the same."""
    qc, qs = _coded(5, 64, 8)
    dc, ds = _coded(6, 64, 9)
    return R.scores(qc, qs, np.concatenate([dc, dc]), np.concatenate([ds, ds]))


def test_topk_equals_the_loops_with_bounds_exclusions_ties_and_padding():
    S = _tied_scores()
    top = S.max(1)
    excl = [[int(np.argmax(S[m]))] if m % 2 else [] for m in range(5)]           # the would-be top hit among them
    for k in (1, 5, 12, 20):
        assert _same(R.topk(S, k), loop_topk(S, k))
        for below in (top, np.nextafter(top, F32(np.inf)), np.nextafter(top, F32(-np.inf))):
            assert _same(R.topk(S, k, excl, below), loop_topk(S, k, excl, below))
    s, i = R.topk(S, 20)
    assert (i[:, 12:] == -1).all() and np.isneginf(s[:, 12:]).all()
    assert all(i[m, 0] < 6 and i[m, 1] == i[m, 0] + 6 for m in range(5))         # ties to the lower id
    s, i = R.topk(S, 3, below=top)
    assert (s < top[:, None]).all()                                              # strict
    s, i = R.topk(S, 12, exclude=excl)
    assert all(excl[m][0] not in i[m] for m in (1, 3)) and (i[1, -1] == -1)


@pytest.mark.parametrize("error", ["non_strict", "ties_up", "drop_exclusions"])
def test_planted_topk_errors_are_caught(error):
    S = _tied_scores()
    top = S.max(1)
    excl = [[int(np.argmax(S[m]))] for m in range(5)]
    want = R.topk(S, 4, excl, np.nextafter(top, F32(np.inf)) if error == "drop_exclusions" else top)
    bel = np.nextafter(top, F32(np.inf)) if error == "drop_exclusions" else top
    assert _same(want, loop_topk(S, 4, excl, bel))
    assert not _same(want, loop_topk(S, 4, excl, bel, **{error: True}))


def test_pipeline_with_candidates_covering_the_corpus_is_the_exact_ranking():
    rng = np.random.default_rng(11)
    Q, D = rng.standard_normal((4, 64)).astype(F32), rng.standard_normal((30, 64)).astype(F32)
    excl = [[0], [], [3, 4], []]
    s, i = R.pipeline(Q, D, 5, rescore_factor=6, exclude=excl)
    S = Q.astype(np.float64) @ D.astype(np.float64).T
    ws, wi = R.topk(S, 5, excl)
    assert np.array_equal(i, wi) and np.allclose(s, ws, rtol=1e-13, atol=0)   # (two float64 summation orders)
    below = np.sort(S, 1)[:, -2]                                                 # the second best score: one survivor above
    s, i = R.pipeline(Q, D, 5, rescore_factor=6, below=below)
    ws, wi = R.topk(S, 5, None, below)
    assert np.array_equal(i, wi) and np.allclose(s, ws, rtol=1e-13, atol=0) and (wi[:, 1:] >= 0).all()


# ---- recall of the scheme ----------------------------------------------------------------------------------------------
def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def _corpus(kind, n, d, rng):
    if kind == "gaussian":
        return _unit(rng.standard_normal((n, d)))
    centres = rng.standard_normal((32, d))
    return _unit(centres[rng.integers(0, 32, n)] + rng.standard_normal((n, d)))


@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("kind", ["gaussian", "mixture"])
def test_recall_of_the_int8_ranking_and_of_the_rescored_pipeline(kind, d):
    """Seed 2024, N = 4000, M = 256, k = 10, unit-norm rows; recall@10 against the float64 ranking of the fp32 rows.
    Measured (int8 alone / rescore_factor 2):  gaussian d = 64: 0.9840 / 1.0000, d = 768: 0.9820 / 1.0000;
    mixture d = 64: 0.9855 / 1.0000, d = 768: 0.9816 / 1.0000."""
    rng = np.random.default_rng(2024)
    D = _corpus(kind, 4000, d, rng)
    Q = _corpus(kind, 256, d, rng)
    k = 10
    exact = R.topk(Q.astype(np.float64) @ D.astype(np.float64).T, k)[1]
    qc, qs = R.quantize(Q)
    dc, ds = R.quantize(D)
    S = R.scores(qc, qs, dc, ds)
    alone = R.recall(R.topk(S, k)[1], exact)
    # (the pipeline at rescore_factor 2, from the same score matrix)
    cand = R.topk(S, 2 * k)[1]
    got = np.empty((256, k), np.int64)
    for m in range(256):
        ids = np.sort(cand[m])
        s = D[ids].astype(np.float64) @ Q[m].astype(np.float64)
        got[m] = ids[np.argsort(-s, kind="stable")[:k]]
    rescored = R.recall(got, exact)
    print(f"{kind} d={d}: recall@10 int8 alone {alone:.4f}, rescore_factor 2 {rescored:.4f}")
    assert alone >= 0.95
    assert rescored >= 0.999
