"""GPU checks of the product quantiser's training and encoding kernels (csrc/pq.hip via contrastors_amd.search) against the numpy
reference tests/pq_ref.py.  Every output is defined bit for bit by that reference (fmaf chains, one subtraction, sums in row
order, one division), so every comparison here is an equality of bits."""
import functools

import numpy as np
import pytest
import torch

from tests import pq_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32


def _bf16_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV).to(torch.bfloat16)


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _same_f32(t, want):
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(want, dtype=F32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _case(d, dsub, n, seed):
    """(rows fp32, shadow) with the half-norm term in play: centroid norms spread over 0.25 .. 2."""
    rng = np.random.default_rng(seed)
    m = d // dsub
    shadow = R.to_bf16(rng.standard_normal((m, R.KSUB, dsub)).astype(F32) * rng.uniform(0.25, 2, (m, R.KSUB, 1)).astype(F32))
    x = rng.standard_normal((n, d)).astype(F32)
    return x, shadow


def _assign(xb, shadow, codes):
    """cx_pq_assign on device views: xb (n, d) bf16 with a row stride, codes (n, m) uint8 with a row stride."""
    from contrastors_amd import _C

    sh = _bf16_dev(shadow)
    hn = torch.from_numpy(R.half_norm(shadow)).to(DEV)
    n, d = xb.shape
    m, _, dsub = shadow.shape
    rc = _C.lib().cx_pq_assign(xb.data_ptr(), n, d, xb.stride(0), sh.data_ptr(), hn.data_ptr(), dsub, codes.data_ptr(),
                               codes.stride(0), _C.cur_stream())
    torch.cuda.synchronize()
    return rc


# ---- cx_pq_assign --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub", [8, 16, 32, 64])
@pytest.mark.parametrize("d", [64, 192, 1024])
def test_pq_encode_equals_the_reference(d, dsub):
    from contrastors_amd.search import pq_encode

    x, shadow = _case(d, dsub, 300, 1000 * d + dsub)
    want = R.assign(x, shadow)                              # rows are independent: one reference for every n
    cb = _bf16_dev(shadow)
    for n in (0, 1, 63, 65, 300):
        got = pq_encode(torch.from_numpy(x[:n]).to(DEV), cb)
        assert got.dtype == torch.uint8 and got.shape == (n, d // dsub) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want[:n])
    got = pq_encode(_bf16_dev(x), shadow)                    # bf16 rows, host codebooks
    assert np.array_equal(got.cpu().numpy(), want)
    hn = R.half_norm(shadow)
    from contrastors_amd.search import _pq_half_norm_device

    assert _same_f32(_pq_half_norm_device(cb), hn)


def test_assign_honours_row_strides_unaligned_rows_and_code_leading_dimensions():
    d, dsub, n = 192, 8, 70
    m = d // dsub
    x, shadow = _case(256, dsub, n, 7)
    wide = _bf16_dev(x)
    for view, cols in ((wide[:, :d], slice(0, d)), (wide[:, 64:], slice(64, 256)), (wide[:, 1: d + 1], slice(1, d + 1)),
                       (wide[3:, 2: d + 2], slice(2, d + 2))):                 # the last two: element loads
        rows = x[n - view.shape[0]:, cols]
        want = R.assign(rows, shadow[:m])
        for ld in (m, m + 5, 64):
            buf = torch.full((view.shape[0], ld), 0xAB, dtype=torch.uint8, device=DEV)
            assert _assign(view, shadow[:m], buf[:, :m]) == 0
            got = buf.cpu().numpy()
            assert np.array_equal(got[:, :m], want) and (got[:, m:] == 0xAB).all()
    # m = 1: ld == m == 1 is legal, the bytes are packed
    x1, sh1 = _case(64, 64, 65, 8)
    buf = torch.full((66,), 0xAB, dtype=torch.uint8, device=DEV)
    assert _assign(_bf16_dev(x1), sh1, buf[:65].view(65, 1)) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[:65], R.assign(x1, sh1)[:, 0]) and got[65] == 0xAB


def test_assign_edge_rows_duplicates_half_norm_winners_extreme_codes_and_single_sub_vectors():
    d, dsub = 192, 8
    m = d // dsub
    _, shadow = _case(d, dsub, 1, 9)
    shadow = shadow.copy()
    shadow[:, 200] = shadow[:, 100]                          # duplicate centroids in every sub-quantiser
    shadow[:, 255] = 0
    shadow[:, 255, 0] = 16                                   # a long centroid ...
    shadow[:, 0] = 0
    shadow[:, 0, 0] = -16                                    # ... and its mirror image
    shadow[:, 50] = 0
    shadow[:, 50, 1] = 1                                     # x . c: 50 -> 1, 51 -> 3;  minus |c|^2 / 2: 0.5 and -1.5
    shadow[:, 51] = 0
    shadow[:, 51, 1] = 3
    rows = []
    for s in range(m):                                       # rows non-zero in one sub-vector only, at every s
        for sub in (shadow[s, 100], 4 * shadow[s, 255], 4 * shadow[s, 0], shadow[s, 50]):
            r = np.zeros(d, F32)
            r[s * dsub: (s + 1) * dsub] = sub
            rows.append(r)
    x = np.stack(rows)
    want = R.assign(x, shadow)
    zero_codes = R.assign(np.zeros((1, d), F32), shadow)[0]  # an all-zero sub-vector: the smallest half norm
    for s in range(m):
        assert want[4 * s: 4 * s + 4, s].tolist() == [100, 255, 0, 50]
        assert (np.delete(want[4 * s: 4 * s + 4], s, axis=1) == np.delete(zero_codes, s)[None, :]).all()
    ip = R.sub_scores(R.to_bf16(x[3:4, :dsub]), shadow[0], np.zeros(R.KSUB, F32))
    assert ip[0, 51] > ip[0, 50]                             # 50 wins through the half-norm term only
    from contrastors_amd.search import pq_encode

    got = pq_encode(torch.from_numpy(x).to(DEV), shadow)
    assert np.array_equal(got.cpu().numpy(), want)


# ---- cx_pq_update --------------------------------------------------------------------------------------------------------
def _update(x, codes, masters, ldc=None):
    from contrastors_amd import _C

    n, d = x.shape
    m, _, dsub = masters.shape
    xb = _bf16_dev(x)
    ldc = m if ldc is None else ldc
    cbuf = torch.zeros(max(n, 1), ldc, dtype=torch.uint8, device=DEV)
    cbuf[:n, :m] = torch.from_numpy(codes).to(DEV)
    ma = torch.from_numpy(masters.copy()).to(DEV)
    sh = torch.full((m, R.KSUB, dsub), 7.0, dtype=torch.bfloat16, device=DEV)
    hn = torch.full((m, R.KSUB), 7.0, dtype=torch.float32, device=DEV)
    rc = _C.lib().cx_pq_update(xb.data_ptr(), n, d, d, cbuf.data_ptr(), ldc, dsub, ma.data_ptr(), sh.data_ptr(), hn.data_ptr(),
                               _C.cur_stream())
    torch.cuda.synchronize()
    assert rc == 0
    return ma, sh, hn


@pytest.mark.parametrize("n, d, dsub", [(1, 64, 8), (255, 64, 16), (257, 192, 8), (257, 64, 64), (1000, 64, 8), (1000, 128, 32),
                                        (1000, 192, 16), (1000, 64, 64)])
def test_update_equals_the_reference(n, d, dsub):
    m = d // dsub
    rng = np.random.default_rng(n + d + dsub)
    x = rng.standard_normal((n, d)).astype(F32) * (2.0 ** rng.integers(-10, 11, (n, 1))).astype(F32)   # spread over 2^20
    codes = rng.integers(0, 40, (n, m)).astype(np.uint8)     # cells 40 .. 255 stay empty
    codes[:, m - 1] = 255                                    # all rows in one cell
    masters = rng.standard_normal((m, R.KSUB, dsub)).astype(F32)
    wm, wsh, whn = R.update(x, codes, masters)
    if n >= 255:
        flipped = R.update(x[::-1], codes[::-1], masters)[0]
        assert not np.array_equal(flipped, wm)               # the order shows on this data
    for ldc in (m, m + 3):
        ma, sh, hn = _update(x, codes, masters, ldc)
        assert _same_f32(ma, wm) and np.array_equal(_bits16(sh), R.bf16_bits(wsh)) and _same_f32(hn, whn)
    assert np.array_equal(wm[:, 40:255], masters[:, 40:255])


def test_update_of_no_rows_is_ok_without_a_launch():
    from contrastors_amd import _C

    ma = torch.ones(8, R.KSUB, 8, device=DEV)
    assert _C.lib().cx_pq_update(None, 0, 64, 64, None, 8, 8, ma.data_ptr(), None, None, _C.cur_stream()) == 0
    assert _C.lib().cx_pq_assign(None, 0, 64, 64, None, None, 8, None, 8, _C.cur_stream()) == 0
    torch.cuda.synchronize()
    assert bool((ma == 1).all())


# ---- training and the index ----------------------------------------------------------------------------------------------
def _check_trained(ix, want):
    wm, wsh, whn = want
    assert ix.is_trained and ix.codebooks.dtype == torch.bfloat16 and ix.codebooks.shape == wm.shape
    assert _same_f32(ix.masters, wm) and np.array_equal(_bits16(ix.codebooks), R.bf16_bits(wsh)) and _same_f32(ix.half_norms, whn)


@pytest.mark.parametrize("d, dsub", [(64, 8), (192, 16)])
def test_train_for_three_iterations_equals_the_reference(d, dsub, tmp_path):
    from contrastors_amd.search import PQFlatIndex, pq_train_rows

    n = 1000
    x = np.random.default_rng(d).standard_normal((n, d)).astype(F32)
    _, first = pq_train_rows(n, None, 3)
    want = R.train(x, first.numpy(), dsub, 3)
    for src in (x, torch.from_numpy(x).to(DEV)):
        ix = PQFlatIndex(d, dsub, device=DEV, seed=3)
        ix.train(src, max_iter=3)
        _check_trained(ix, want)
    rows, first = pq_train_rows(n, 600, 3)                   # a seeded sample, gathered on the host for host sources
    want = R.train(x[rows.numpy()], first.numpy(), dsub, 3)
    np.save(tmp_path / "x.npy", x)
    for src in (x, torch.from_numpy(x).to(DEV), np.load(tmp_path / "x.npy", mmap_mode="r")):
        ix = PQFlatIndex(d, dsub, device=DEV, seed=3)
        ix.train(src, max_iter=3, sample=600)
        _check_trained(ix, want)
    ix = PQFlatIndex(d, dsub, device=DEV)                    # given codebooks are the masters
    ix.train(codebooks=want[0])
    _check_trained(ix, (want[0], R.to_bf16(want[0]), R.half_norm(R.to_bf16(want[0]))))
    ix0 = PQFlatIndex(d, dsub, device=DEV, seed=3)           # no iterations: the initial rows
    ix0.train(x, max_iter=0)
    init = R.init_masters(x, pq_train_rows(n, None, 3)[1].numpy(), dsub)
    _check_trained(ix0, (init, init, R.half_norm(init)))


def test_uneven_adds_codes_and_float_rows_give_the_same_index_and_decode_is_the_concatenation(tmp_path):
    from contrastors_amd.search import PQFlatIndex, pq_encode

    d, dsub, N = 192, 8, 700
    m = d // dsub
    D, shadow = _case(d, dsub, N, 11)
    want = R.assign(D, shadow)
    np.save(tmp_path / "D.npy", D)

    def fresh():
        ix = PQFlatIndex(d, dsub, device=DEV)
        ix.train(codebooks=shadow)
        return ix

    one = fresh()
    one.add(D)
    assert one.ntotal == N and one.codes.shape == (N, m) and one.codes.dtype == torch.uint8
    assert np.array_equal(one.codes.cpu().numpy(), want)
    three = fresh()
    three.add(D[:1])
    three.add(torch.from_numpy(D[1:130]).to(DEV))
    three.add(np.load(tmp_path / "D.npy", mmap_mode="r")[130:])
    assert np.array_equal(three.codes.cpu().numpy(), want)
    coded = fresh()
    coded.reserve(N)
    ptr = coded._store.data_ptr()
    coded.add(want[:300])
    coded.add(pq_encode(torch.from_numpy(D[300:]).to(DEV), one.codebooks))
    assert coded._store.data_ptr() == ptr and np.array_equal(coded.codes.cpu().numpy(), want)
    dec = one.decode()
    assert dec.dtype == torch.bfloat16 and dec.shape == (N, d)
    assert np.array_equal(_bits16(dec), R.bf16_bits(R.decode(want, shadow)))
    ids = [5, 699, 0, 5]
    assert np.array_equal(_bits16(one.decode(ids)), R.bf16_bits(R.decode(want[ids], shadow)))
    with pytest.raises(ValueError, match="ids in"):
        one.decode([700])
    assert one.batch_rows(33, 20) == 33
    with pytest.raises(RuntimeError, match="reset"):
        one.train(codebooks=shadow)
    one.reset()
    assert one.ntotal == 0 and one.codes.shape == (0, m) and one.is_trained and one.decode().shape == (0, d)
    one.add(D[:10])                                          # the codebooks stayed
    assert np.array_equal(one.codes.cpu().numpy(), want[:10])
