"""cx_search_pq_window_topk against tests/ivf_pq_ref.py, by equality.  Every (q, n) acc comes from FlatIPIndex(decode(codes))
.search(Q, k = N) scattered into an (M, N) matrix (N <= 1024); bias, window, below, exclusions, order and padding are numpy."""
import numpy as np
import pytest
import torch

from tests import ivf_pq_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(DEV, dtype).contiguous()


def pq_window(Q, codes, cb, k, mid=None, end=None, bias=None, exclude=None, below=None):
    """Device Q (M, d) bf16, codes (N, m) uint8 (any row stride / base), cb (m, 256, dsub) bf16 -> numpy (scores, ids)."""
    from contrastors_amd import _C

    h = _C.lib()
    M, N, (m, _, dsub) = Q.shape[0], codes.shape[0], cb.shape
    xptr = xids = None
    if exclude is not None:
        xptr = _dev(np.cumsum([0] + [len(e) for e in exclude]), torch.int64)
        xids = _dev(np.concatenate([np.asarray(e, np.int64) for e in exclude] + [np.zeros(1, np.int64)]), torch.int64)
    mid, end, bias, below = _dev(mid, torch.int64), _dev(end, torch.int64), _dev(bias, torch.float32), _dev(below, torch.float32)
    ws = torch.empty(h.cx_search_pq_window_ws_bytes(M, k) + 16, dtype=torch.uint8, device=DEV)
    s = torch.empty(M, k, dtype=torch.float32, device=DEV)
    i = torch.empty(M, k, dtype=torch.int64, device=DEV)
    _C.check(h.cx_search_pq_window_topk(Q.data_ptr(), codes.data_ptr(), cb.data_ptr(), M, N, m * dsub, dsub, m * dsub,
                                        codes.stride(0) if N > 1 else m, k, _C.ptr(mid), _C.ptr(end), _C.ptr(bias), _C.ptr(xptr),
                                        _C.ptr(xids), _C.ptr(below), ws.data_ptr(), s.data_ptr(), i.data_ptr(), _C.cur_stream()))
    return s.cpu().numpy(), i.cpu().numpy()


def make(M, N, d, dsub, seed=0):
    """-> device (Q, codes, cb, decoded rows) and the numpy acc (M, N); code rows 1 and N - 1 repeat row 0 (ties)."""
    from contrastors_amd.search import FlatIPIndex

    g = torch.Generator().manual_seed(1000 * M + N + d + dsub + seed)
    m = d // dsub
    Q = torch.randn(M, d, generator=g).to(DEV, torch.bfloat16)
    cb = torch.randn(m, 256, dsub, generator=g).to(DEV, torch.bfloat16)
    codes = torch.randint(0, 256, (N, m), generator=g, dtype=torch.uint8)
    if N:
        codes[1 % N], codes[N - 1] = codes[0], codes[0]
    codes = codes.to(DEV)
    dec = cb[torch.arange(m, device=DEV)[None, :], codes.long()].reshape(N, d)
    acc = torch.empty(M, N, dtype=torch.float32, device=DEV)
    if M and N:
        ix = FlatIPIndex(d, device=DEV)
        ix.add(dec)
        s, i = ix.search(Q, N)
        acc.scatter_(1, i, s)
    return Q, codes, cb, dec, acc.cpu().numpy()


def windows(M, N):
    """Query tile 0 mixes every kind of window, the ends of the corpus among them; tile 1 (rows 128 - 255) is all empty; the
    rows after it are random."""
    rng = np.random.default_rng(M + N)
    kinds = [(5, 5), None, (126, 130), (-1, N), (-7, N + 50), (-1, 3), (N - 4, N), (N + 3, N + 9)]
    mid, end = rng.integers(-3, N + 3, M), rng.integers(-3, N + 3, M)
    for r in range(min(M, 256)):
        kind = kinds[r % len(kinds)] if r < 128 else (r, r)
        mid[r], end[r] = kind if kind is not None else (r % N - 1, r % N + 1)          # one row
    return mid.astype(np.int64), end.astype(np.int64)


@pytest.mark.parametrize("d, dsub", [(64, 8), (192, 16), (192, 64)])
@pytest.mark.parametrize("N", [1, 127, 129, 300, 1000])
@pytest.mark.parametrize("M", [1, 129, 300])
def test_window_bias_below_exclude_against_the_reference(M, N, d, dsub):
    Q, codes, cb, dec, acc = make(M, N, d, dsub)
    mid, end = windows(M, N)
    bias = ((np.arange(M) % 5 - 2) * 0.37).astype(np.float32)     # distinct per row; negative, zero and positive
    for k in (1, 10, 200):
        gs, gi = pq_window(Q, codes, cb, k, mid, end, bias)
        ws, wi = V.window_topk(acc, bias, k, mid, end)
        assert np.array_equal(gi, wi) and np.array_equal(_bits(gs), _bits(ws)), k
    # the whole corpus for every row (NULL windows): rows 0, 1 and N - 1 tie, lower id first
    gs, gi = pq_window(Q, codes, cb, 10, bias=bias)
    ws, wi = V.window_topk(acc, bias, 10)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gs), _bits(ws))
    # below between a row's biased and unbiased best score: only the rows with a negative bias keep that hit; and the top hit
    # of the unfiltered search excluded
    below = (acc.max(1) + np.float32(0.1)).astype(np.float32)
    top = V.window_topk(acc, bias, 1, mid, end)[1][:, 0]
    exclude = [[t] if t >= 0 else [] for t in top]
    gs, gi = pq_window(Q, codes, cb, 10, mid, end, bias, exclude, below)
    ws, wi = V.window_topk(acc, bias, 10, mid, end, exclude, below)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gs), _bits(ws))


@pytest.mark.parametrize("M, N, d, dsub", [(129, 300, 64, 8), (300, 1000, 192, 16), (1, 129, 192, 64)])
def test_null_bias_is_the_bf16_window_kernel_over_the_decoded_rows(M, N, d, dsub):
    from contrastors_amd import _C

    Q, codes, cb, dec, acc = make(M, N, d, dsub, seed=1)
    mid, end = windows(M, N)
    h = _C.lib()
    ws = torch.empty(h.cx_search_window_ws_bytes(M, 10) + 16, dtype=torch.uint8, device=DEV)
    s = torch.empty(M, 10, dtype=torch.float32, device=DEV)
    i = torch.empty(M, 10, dtype=torch.int64, device=DEV)
    tm, te = _dev(mid, torch.int64), _dev(end, torch.int64)
    _C.check(h.cx_search_window_topk(Q.data_ptr(), dec.data_ptr(), M, N, d, d, d, 10, tm.data_ptr(), te.data_ptr(), None, None,
                                     None, ws.data_ptr(), s.data_ptr(), i.data_ptr(), _C.cur_stream()))
    gs, gi = pq_window(Q, codes, cb, 10, mid, end)
    assert np.array_equal(gi, i.cpu().numpy()) and np.array_equal(_bits(gs), _bits(s.cpu().numpy()))
    ws_, wi = V.window_topk(acc, None, 10, mid, end)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gs), _bits(ws_))
    # the byte path: code rows with a leading dimension and an unaligned base give the same result
    wide = torch.zeros(N * (codes.shape[1] + 3) + 1, dtype=torch.uint8, device=DEV)
    view = wide[1:].view(N, codes.shape[1] + 3)[:, : codes.shape[1]]
    view.copy_(codes)
    bias = np.linspace(-1, 1, M).astype(np.float32)
    for b in (None, bias):
        a, c = pq_window(Q, view, cb, 10, mid, end, b), pq_window(Q, codes, cb, 10, mid, end, b)
        assert np.array_equal(a[1], c[1]) and np.array_equal(_bits(a[0]), _bits(c[0]))


@pytest.mark.parametrize("M, N", [(0, 300), (5, 0)])
def test_empty_operands(M, N):
    Q, codes, cb, dec, acc = make(M, N, 64, 8)
    gs, gi = pq_window(Q, codes, cb, 7, bias=np.ones(M, np.float32))
    assert gs.shape == (M, 7) and np.all(gs == -np.inf) and np.all(gi == -1)
