"""The draw rule of cx_mlm_mask (contrastors_amd/csrc/mlm_mask.hip) restated in numpy: the yardstick the GPU
tests compare the kernel with element for element.  tests/test_mlm_data_cpu.py checks the restatement itself: against the
published Philox4x32-10 test vectors, against planted errors, and for the rates the rule promises.

`flaw` plants one error in the rule (the CPU test shows that each is caught): "counter" swaps two counter words, "swap" uses
u1 for the target draw and u0 for the split, "split" takes 0.9 for the 0.8 threshold.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words; key: two python ints.  Returns four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def threshold(x):
    """T(x) = (uint32) fminf(x * 2^32, 4294967040.f) in fp32 arithmetic."""
    return np.uint64(min(np.float32(x) * np.float32(4294967296.0), np.float32(4294967040.0)))


def draws(n_tokens, seed, offset, flaw=None):
    """(u0, u1, u2) of the flat positions 0 .. n_tokens - 1 under (seed, offset)."""
    g = np.arange(n_tokens, dtype=np.uint64)
    off = np.full(n_tokens, offset, dtype=np.uint64)
    counter = [g & LO, g >> S32, off & LO, off >> S32]
    if flaw == "counter":
        counter[0], counter[1] = counter[1], counter[0]
    u0, u1, u2, _ = philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return u0, u1, u2


def specialness(ids, attention_mask=None, special_mask=None, special_ids=()):
    sp = np.zeros(ids.shape, dtype=bool)
    if attention_mask is not None:
        sp |= np.asarray(attention_mask) == 0
    if special_mask is not None:
        sp |= np.asarray(special_mask) != 0
    if len(special_ids):
        sp |= np.isin(ids, np.asarray(special_ids, dtype=np.int64))
    return sp


def mlm_mask(ids, p, seed, offset, mask_token_id, random_vocab, attention_mask=None, special_mask=None, special_ids=(),
             flaw=None, u=None):
    """ids (B, S) any integer dtype -> (out_ids, labels) int64, by the rule.  `u` = draws(...) computed earlier, to share."""
    ids = np.ascontiguousarray(ids).astype(np.int64)
    u0, u1, u2 = draws(ids.size, seed, offset, flaw) if u is None else u
    if flaw == "swap":
        u0, u1 = u1, u0
    u0, u1, u2 = (x.reshape(ids.shape) for x in (u0, u1, u2))
    special = specialness(ids, attention_mask, special_mask, special_ids)
    target = ~special & (u0 < threshold(p))
    to_mask = u1 < threshold(0.9 if flaw == "split" else 0.8)
    to_word = ~to_mask & (u1 < threshold(0.9))
    words = ((u2 * np.uint64(random_vocab)) >> S32).astype(np.int64)
    out = np.where(target & to_mask, np.int64(mask_token_id), np.where(target & to_word, words, ids))
    labels = np.where(target, ids, np.int64(-100))
    return out, labels
