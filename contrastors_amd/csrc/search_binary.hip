// search_binary.hip -- the binary (sign-bit) side of the curation search: packing embeddings into sign codes, a fused Hamming
// top-k over packed codes (faiss IndexBinaryFlat.search; sentence-transformers "ubinary") and the exact re-scoring of a
// candidate list against the bf16 rows.  Coarse Hamming top-(k R) + cx_rescore_topk is the standard pipeline for models
// trained with `hamming: true`; it brings a corpus that does not fit HBM as bf16 (1536 B per 768-d row) onto one card
// (96 B per row).
//
// cx_search_hamming_topk has the structure of search.hip (128 x 128 tiles, a sorted running list per (row, split), the k-th
// entry as a register threshold, a rank-counting merge); what differs is the score.  A code bit b is expanded IN THE KERNEL
// to the int8 value +64 (b = 0) or -64 (b = 1) -- the two differ in the sign bit only, so a dword of four values is one shift
// and one v_and_or_b32 -- and the tile runs on v_mfma_i32_16x16x64_i8:  acc = 4096 (d - 2 hamming), exact in int32
// (|acc| <= 2^22).  i8 rather than fp4 (v_mfma_scale_f32_16x16x128_f8f6f4): its K of 64 divides every supported d, so the
// only padding is the unused half of the last 128-wide LDS chunk; the accumulator is an integer, so "exact" needs no argument
// about fp32; and the expansion to fp4 nibbles costs the same VALU work for half the LDS bytes, which is not where this kernel
// spends its time (scripts/search_binary_microbench.py, DESIGN.md "Binary index").
// The K position a code bit lands on is a fixed permutation, THE SAME for the query and the document operand (both go through
// expand()), and a dot product does not see a permutation applied to both sides; what has to be right is which ROW a lane
// feeds (lane & 15, as for every 16x16 MFMA) and where the result lands (column lane & 15, rows 4 (lane >> 4) + r).
// tests/test_binary_search_gpu.py places single set bits against asymmetric codes to pin this.
//
// Order: ascending distance, ties to the lower id -- a strict total order, so the result is the unique top-k whatever the
// split count.  Integer distances tie all the time: an entry equal to a full list's k-th distance cannot enter (its id is
// larger: ids grow along a split, and the candidates of one tile are ranked together before they meet the list), and the
// split merge ranks by (distance, id).  No atomics; the (M, N) distances are never written.
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

#include <limits.h>

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;

constexpr int TM = 128, TN = 128;
constexpr int BKD = 128;             // code bits (= int8 K elements) per LDS chunk: 16 code bytes -> 128 operand bytes per row
constexpr int PANEL = TM * BKD;      // 16 KiB: one operand's chunk
constexpr int MAXK = 1024;
constexpr int MAXSPLIT = 64;
constexpr long MAX_N = 0x7fffffffL - TN;   // int column indices of the last tile
constexpr int SPLIT_TARGET_WG = 512;
constexpr int UNIT = 4096;           // (+-64)^2: acc = UNIT * (d - 2 * distance)

struct HCand {
    int dist;
    int id;
};

CX_DEVICE bool beats(HCand a, HCand b) { return a.dist < b.dist || (a.dist == b.dist && a.id < b.id); }

// [128 rows][8 chunks of 16 B]: chunk c of row r at r*128 + ((c ^ (r & 7)) << 4)
CX_DEVICE int poff(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

CX_DEVICE void wave_sync() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

struct HammingParams {
    const uint8_t* Q;
    const uint8_t* D;
    long ldq, ldd;         // bytes
    int M, N, d, k;
    int nsplit, tiles_n, tiles_per_split;
    const int64_t* xptr;
    const int64_t* xids;
    const int32_t* maxd;   // (M) inclusive upper bound on the distance, or null
    HCand* lists;          // (M, nsplit, k)
    int* counts;           // (M, nsplit)
};

// thread tid stages 128 code bits of one row: query row tid (tid < 128) or document row tid - 128
CX_DEVICE void stage(const HammingParams& p, int m0, int n0, int kc, int tid, uint2 (&w)[2]) {
    const int r = tid & 127;
    const uint8_t* row = (tid < 128) ? p.Q + (int64_t)min(m0 + r, p.M - 1) * p.ldq
                                     : p.D + (int64_t)min(n0 + r, p.N - 1) * p.ldd;   // clamped rows are never admitted
    const int b0 = kc * (BKD / 8);
    w[0] = *reinterpret_cast<const uint2*>(row + b0);
    w[1] = (b0 + 8 < p.d / 8) ? *reinterpret_cast<const uint2*>(row + b0 + 8) : make_uint2(0u, 0u);
}
// bits j, j + 8, j + 16, j + 24 of a code word -> the four int8 values of dword j: +64, or -64 where the bit is set
CX_DEVICE uint32_t expand(uint32_t w, int j) { return ((w << (7 - j)) & 0x80808080u) | 0x40404040u; }
CX_DEVICE void commit(char* qbuf, char* dbuf, int tid, const uint2 (&w)[2], bool second) {
    char* buf = (tid < 128) ? qbuf : dbuf;
    const int r = tid & 127;
    const uint32_t words[4] = {w[0].x, w[0].y, w[1].x, w[1].y};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t v = words[i];
        uint4 lo = make_uint4(expand(v, 0), expand(v, 1), expand(v, 2), expand(v, 3));
        uint4 hi = make_uint4(expand(v, 4), expand(v, 5), expand(v, 6), expand(v, 7));
        if (i >= 2 && !second) lo = hi = make_uint4(0u, 0u, 0u, 0u);   // past d: zeros (the K loop does not read them either)
        *reinterpret_cast<uint4*>(buf + poff(r, 2 * i)) = lo;
        *reinterpret_cast<uint4*>(buf + poff(r, 2 * i + 1)) = hi;
    }
}

CX_DEVICE int count_beating(const HCand* L, int n, HCand e) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beats(L[mid], e)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

constexpr int PEND = 32;           // admitted candidates a row collects in LDS before they are merged into its list

struct HammingLds {
    char ops[4 * PANEL];          // [Q, D] x 2 chunk buffers; after the K loop: the 128 x 128 int32 accumulator tile
    HCand mbuf[4][MAXK];          // per wave: the merged list being built
    HCand pend[TM][PEND];         // per row: admitted candidates not merged yet
    HCand cand[4][PEND + TN];     // per wave: the candidates of one merge (the tile's new ones, then the row's pending ones)
    HCand sorted[4][PEND + TN];   // ... and ranked
    int thr[TM], bel[TM];         // in accumulator units: admissible = acc > thr (strictly nearer than the k-th) && acc >= bel
    int cnt[TM], flag[TM], pcnt[TM];
    int any;
};

CX_DEVICE int acc_of_dist(int d, int dist) { return UNIT * (d - 2 * dist); }

// one wave: merge the c candidates in L.cand[wave] into the row's running list (rank counting), refresh its threshold
CX_DEVICE void merge_row(const HammingParams& p, HammingLds& L, int row, int m, int split, int wave, int lane, int c) {
    const HCand* cand = L.cand[wave];
    HCand* srt = L.sorted[wave];
    HCand* mb = L.mbuf[wave];
    const int cnt = L.cnt[row];
    for (int i = lane; i < c; i += 64) {
        const HCand e = cand[i];
        int r = 0;
        for (int j = 0; j < c; ++j) r += beats(cand[j], e) ? 1 : 0;
        srt[r] = e;
    }
    wave_sync();
    HCand* list = p.lists + ((int64_t)m * p.nsplit + split) * p.k;
    for (int j = lane; j < cnt; j += 64) {
        const HCand e = list[j];
        const int pos = j + count_beating(srt, c, e);
        if (pos < p.k) mb[pos] = e;
    }
    for (int i = lane; i < c; i += 64) {
        const HCand e = srt[i];
        const int pos = i + count_beating(list, cnt, e);
        if (pos < p.k) mb[pos] = e;
    }
    wave_sync();
    const int ncnt = min(p.k, cnt + c);
    for (int j = lane; j < ncnt; j += 64) list[j] = mb[j];
    if (lane == 0) {
        L.cnt[row] = ncnt;
        L.pcnt[row] = 0;
        // full list: only a strictly smaller distance can still enter (an equal one has a larger id)
        if (ncnt == p.k) L.thr[row] = acc_of_dist(p.d, mb[p.k - 1].dist);
    }
    wave_sync();
}

// one wave: the admissible entries of tile row `row` join the row's pending candidates; a merge into the list in global
// memory (a chain of dependent loads) happens only when they no longer fit.  Between merges the row's threshold is the k-th
// distance of an OLDER list: it admits more than the current one would, never less, and what it admits wrongly ranks past k in
// the next merge.
CX_DEVICE void insert_row(const HammingParams& p, HammingLds& L, const int* tile, int row, int m, int n0, int split, int wave,
                          int lane) {
    const int thr = L.thr[row], bel = L.bel[row], pc = L.pcnt[row];
    const int64_t x0 = p.xptr ? p.xptr[m] : 0, x1 = p.xptr ? p.xptr[m + 1] : 0;
    bool ok[2];
    int pos[2], c = 0;
    HCand e[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h, n = n0 + j;
        const int a = tile[row * TN + j];
        ok[h] = n < p.N && a > thr && a >= bel;
        if (ok[h])
            for (int64_t x = x0; x < x1; ++x)
                if (p.xids[x] == n) ok[h] = false;
        const unsigned long long mask = __ballot(ok[h]);
        pos[h] = c + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
        e[h] = HCand{(UNIT * p.d - a) >> 13, n};
        c += __popcll(mask);
    }
    if (c == 0) return;
    if (pc + c <= PEND) {   // the common case: one or two new candidates, straight into the row's pending slots
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (ok[h]) L.pend[row][pc + pos[h]] = e[h];
        if (lane == 0) L.pcnt[row] = pc + c;
        wave_sync();
        return;
    }
    HCand* cand = L.cand[wave];
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (ok[h]) cand[pos[h]] = e[h];
    if (lane < pc) cand[c + lane] = L.pend[row][lane];
    wave_sync();
    merge_row(p, L, row, m, split, wave, lane, c + pc);
}

__global__ __launch_bounds__(256, 1) void hamming_tiles_kernel(HammingParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    HammingLds& L = *reinterpret_cast<HammingLds*>(dsm);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int tm = blockIdx.x / p.nsplit, split = blockIdx.x % p.nsplit;
    const int m0 = tm * TM;
    const int t_begin = split * p.tiles_per_split, t_end = min(p.tiles_n, t_begin + p.tiles_per_split);
    const int nk = (p.d + BKD - 1) / BKD;

    if (tid < TM) {
        const int m = m0 + tid;
        L.thr[tid] = m < p.M ? INT_MIN : INT_MAX;   // rows past M never pass the threshold test
        int bel = INT_MIN;
        if (m < p.M && p.maxd) {
            const int md = p.maxd[m];
            bel = md < 0 ? INT_MAX : acc_of_dist(p.d, min(md, p.d));
        }
        L.bel[tid] = bel;
        L.cnt[tid] = 0;
        L.flag[tid] = 0;
        L.pcnt[tid] = 0;
    }
    if (tid == 0) L.any = 0;
    __syncthreads();

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * TN;
        i32x4_t acc[4][4];   // [query block][document block]
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = i32x4_t{0, 0, 0, 0};
        uint2 w[2];
        stage(p, m0, n0, 0, tid, w);
        commit(L.ops, L.ops + PANEL, tid, w, 64 < p.d);
        __syncthreads();
        for (int kc = 0; kc < nk; ++kc) {
            const char* qb_ = L.ops + (kc & 1) * 2 * PANEL;
            const char* db_ = qb_ + PANEL;
            const int kn = min(kc + 1, nk - 1);   // the last chunk is staged twice (unconditional loads)
            stage(p, m0, n0, kn, tid, w);
            const int nks = (p.d - kc * BKD) > 64 ? 2 : 1;
            for (int ks = 0; ks < nks; ++ks) {
                i32x4_t fq[4], fd[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    fq[b] = *reinterpret_cast<const i32x4_t*>(qb_ + poff(wq * 64 + b * 16 + l15, ks * 4 + lh));
                    fd[b] = *reinterpret_cast<const i32x4_t*>(db_ + poff(wd * 64 + b * 16 + l15, ks * 4 + lh));
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fd[b], fq[a], acc[a][b], 0, 0, 0);
            }
            char* nq = L.ops + ((kc + 1) & 1) * 2 * PANEL;
            commit(nq, nq + PANEL, tid, w, kn * BKD + 64 < p.d);
            __syncthreads();
        }

        // acc[a][b][r] = UNIT * (d - 2 hamming(query m0 + wq*64 + a*16 + l15, document n0 + wd*64 + b*16 + 4*lh + r))
        bool hit = false;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int row = wq * 64 + a * 16 + l15;
            const int thr = L.thr[row], bel = L.bel[row];
            bool h = false;
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int v = acc[a][b][r];
                    h |= (v > thr) & (v >= bel) & (n0 + wd * 64 + b * 16 + 4 * lh + r < p.N);
                }
            if (h) L.flag[row] = 1;
            hit |= h;
        }
        if (hit) L.any = 1;
        __syncthreads();
        if (L.any) {
            int* tile = reinterpret_cast<int*>(L.ops);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    *reinterpret_cast<i32x4_t*>(tile + (wq * 64 + a * 16 + l15) * TN + wd * 64 + b * 16 + 4 * lh) = acc[a][b];
            __syncthreads();
            // this wave's flagged rows (row = wave + 4 i) as one mask: one LDS round trip instead of one per row
            unsigned long long todo = __ballot(lane < TM / 4 && L.flag[wave + 4 * (lane & (TM / 4 - 1))] != 0);
            while (todo) {
                const int row = wave + 4 * (__ffsll(todo) - 1);
                todo &= todo - 1;
                insert_row(p, L, tile, row, m0 + row, n0, split, wave, lane);
            }
            __syncthreads();
            if (tid < TM) L.flag[tid] = 0;
            if (tid == 0) L.any = 0;
        }
        __syncthreads();
    }
    // what is still pending goes into the lists
    for (int row = wave; row < TM; row += 4) {
        const int pc = L.pcnt[row];
        if (pc == 0) continue;
        if (lane < pc) L.cand[wave][lane] = L.pend[row][lane];
        wave_sync();
        merge_row(p, L, row, m0 + row, split, wave, lane, pc);
    }
    __syncthreads();
    if (tid < TM && m0 + tid < p.M) p.counts[(int64_t)(m0 + tid) * p.nsplit + split] = L.cnt[tid];
}

// one wave per query row: merge the row's nsplit sorted lists into its top-k
__global__ __launch_bounds__(256) void hamming_merge_kernel(const HCand* __restrict__ lists, const int* __restrict__ counts,
                                                            int M, int nsplit, int k, int32_t* __restrict__ out_d,
                                                            int64_t* __restrict__ out_id) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const HCand* base = lists + (int64_t)row * nsplit * k;
    const int* cnt = counts + (int64_t)row * nsplit;
    int total = 0;
    for (int s = 0; s < nsplit; ++s) total += cnt[s];
    for (int idx = lane; idx < nsplit * k; idx += 64) {
        const int s = idx / k, j = idx - s * k;
        if (j >= cnt[s]) continue;
        const HCand e = base[(int64_t)s * k + j];
        int rank = j;
        for (int s2 = 0; s2 < nsplit && rank < k; ++s2)
            if (s2 != s) rank += count_beating(base + (int64_t)s2 * k, cnt[s2], e);
        if (rank < k) {
            out_d[(int64_t)row * k + rank] = e.dist;
            out_id[(int64_t)row * k + rank] = e.id;
        }
    }
    for (int r = min(total, k) + lane; r < k; r += 64) {
        out_d[(int64_t)row * k + r] = INT_MAX;
        out_id[(int64_t)row * k + r] = -1;
    }
}

int auto_splits(int M, long N, int nsplit) {
    const int tiles_m = (M + TM - 1) / TM;
    const long tiles_n = (N + TN - 1) / TN;
    if (nsplit <= 0) nsplit = (SPLIT_TARGET_WG + tiles_m - 1) / tiles_m;
    nsplit = min(nsplit, MAXSPLIT);
    return (int)max(1L, min((long)nsplit, tiles_n));
}

// ---- sign packing: one wave per 64 consecutive dimensions of a row ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pack_sign_kernel(const T* __restrict__ X, long ldx, long units, int upr,
                                                        uint8_t* __restrict__ out, long ldo) {
    const int lane = threadIdx.x & 63;
    const long nwaves = (long)gridDim.x * 4;
    for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += nwaves) {
        const long row = u / upr;
        const int c = (int)(u - row * upr);
        const T raw = X[row * ldx + c * 64 + lane];
        float v;
        if constexpr (sizeof(T) == 2) v = bf16_to_f32(raw); else v = raw;
        const unsigned long long mask = __ballot(v > 0.f);   // +-0 and NaN compare false
        // numpy.packbits: dimension 8 b + i is bit 7 - i of byte b = the big-endian bytes of the bit-reversed mask
        const unsigned long long rev = __brevll(mask);
        if (lane < 8) out[row * ldo + c * 8 + lane] = (uint8_t)(rev >> (8 * (7 - lane)));
    }
}

// ---- exact re-scoring of candidate lists ----------------------------------------------------------------------------
constexpr int MAXC = 4096;

// One workgroup per query.  Scores: 16 candidates at a time as the A rows of v_mfma_f32_16x16x32_bf16 against the query in
// every B column, K walked 32 at a time from 0 -- the instruction and the K order of search.hip, so the score of a pair has
// the bits cx_search_topk gives it (1 / 16 of the tile is used; the stage is bound by the row gather).  Then every candidate
// counts the ones that beat it in (score descending, id ascending, position ascending): its rank.
__global__ __launch_bounds__(256) void rescore_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ D,
                                                      const int64_t* __restrict__ cand, const int64_t* __restrict__ ids,
                                                      long R, int d, long ldq, long ldd, int c, int k,
                                                      const float* __restrict__ below, float* __restrict__ out_s,
                                                      int64_t* __restrict__ out_id) {
    __shared__ float sc[MAXC];
    __shared__ int64_t sid[MAXC];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lh = lane >> 4;
    const bf16_t* q = Q + (int64_t)m * ldq;
    const int64_t* crow = cand + (int64_t)m * c;
    const float bel = below ? below[m] : INFINITY;
    for (int g = wave; g * 16 < c; g += 4) {
        const int j = g * 16 + l15;
        const int64_t r = j < c ? crow[j] : -1;
        const bf16_t* drow = (r >= 0 && r < R) ? D + r * ldd : q;   // skipped entries read the query: always mapped
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < d; k0 += 32) {
            const bf16x8_t fd = *reinterpret_cast<const bf16x8_t*>(drow + k0 + lh * 8);
            const bf16x8_t fq = *reinterpret_cast<const bf16x8_t*>(q + k0 + lh * 8);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd, fq, acc, 0, 0, 0);
        }
        // acc[e] = score of candidate g*16 + 4*lh + e (the same in every column l15)
        if (l15 == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int jj = g * 16 + 4 * lh + e;
                if (jj < c) {
                    const int64_t rr = crow[jj];
                    const bool ok = rr >= 0 && rr < R && acc[e] < bel;
                    sc[jj] = acc[e];
                    sid[jj] = ok ? (ids ? ids[(int64_t)m * c + jj] : rr) : -1;
                }
            }
        }
    }
    __syncthreads();
    int nv = 0;
    for (int j0 = 0; j0 < c; j0 += 256) {
        const int j = j0 + tid;
        const bool valid = j < c && sid[j] >= 0;
        nv += __syncthreads_count(valid);
        if (!valid) continue;
        const float s = sc[j];
        const int64_t id = sid[j];
        int rank = 0;
        for (int t = 0; t < c; ++t) {
            const float st = sc[t];
            const int64_t it = sid[t];
            const bool b = st > s || (st == s && (it < id || (it == id && t < j)));
            rank += (it >= 0 && b) ? 1 : 0;
        }
        if (rank < k) {
            out_s[(int64_t)m * k + rank] = s;
            out_id[(int64_t)m * k + rank] = id;
        }
    }
    for (int r = min(nv, k) + tid; r < k; r += 256) {
        out_s[(int64_t)m * k + r] = -INFINITY;
        out_id[(int64_t)m * k + r] = -1;
    }
}

}  // namespace

extern "C" {

int cx_pack_sign_bits(const void* X, int dtype, long rows, int d, long ldx, uint8_t* out, long ldo, void* stream) {
    if (rows < 0 || d < 64 || d > 1024 || (d % 64) != 0) return CX_ERR_SHAPE;
    if (dtype != 0 && dtype != 1) return CX_ERR_ARG;
    if (rows == 0) return CX_OK;
    if (!X || !out) return CX_ERR_ARG;
    if (ldx < d || ldo < d / 8) return CX_ERR_ALIGN;
    const int upr = d / 64;
    const long units = rows * upr;
    const int grid = (int)min((units + 3) / 4, 1L << 16);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        hipLaunchKernelGGL(pack_sign_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)X, ldx, units, upr, out, ldo);
    else
        hipLaunchKernelGGL(pack_sign_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)X, ldx, units, upr, out, ldo);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

long cx_search_hamming_ws_bytes(int M, long N, int k, int nsplit) {
    if (M <= 0 || N <= 0 || k <= 0) return 0;
    const long s = auto_splits(M, N, nsplit);
    return (long)M * s * ((long)k * (long)sizeof(HCand) + (long)sizeof(int)) + 16;
}

int cx_search_hamming_topk(const uint8_t* Qc, const uint8_t* Dc, int M, long N, int d, long ldq, long ldd, int k,
                           const int64_t* excl_ptr, const int64_t* excl_ids, const int32_t* max_dist, int nsplit, void* ws,
                           int32_t* out_dist, int64_t* out_ids, void* stream) {
    if (M < 0 || N < 0 || k < 1 || k > MAXK || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!Qc || !out_dist || !out_ids || (N > 0 && (!Dc || !ws)) || (excl_ptr && !excl_ids)) return CX_ERR_ARG;
    if (ldq < d / 8 || (ldq % 8) != 0 || (N > 0 && (ldd < d / 8 || (ldd % 8) != 0))) return CX_ERR_ALIGN;
    if (((uintptr_t)Qc & 7) || ((uintptr_t)Dc & 7) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int ns = N > 0 ? auto_splits(M, N, nsplit) : 1;
    HCand* lists = reinterpret_cast<HCand*>(ws);
    int* counts = N > 0 ? reinterpret_cast<int*>(lists + (int64_t)M * ns * k) : nullptr;
    if (N > 0) {
        HammingParams p = {};
        p.Q = Qc; p.D = Dc; p.ldq = ldq; p.ldd = ldd;
        p.M = M; p.N = (int)N; p.d = d; p.k = k;
        p.nsplit = ns;
        p.tiles_n = (int)((N + TN - 1) / TN);
        p.tiles_per_split = (p.tiles_n + ns - 1) / ns;
        p.xptr = excl_ptr; p.xids = excl_ids; p.maxd = max_dist;
        p.lists = lists; p.counts = counts;
        const int tiles_m = (M + TM - 1) / TM;
        static CxLdsOptIn opt;
        if (!opt.ensure(reinterpret_cast<const void*>(&hamming_tiles_kernel), (int)sizeof(HammingLds))) return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(hamming_tiles_kernel, dim3(tiles_m * ns), dim3(256), sizeof(HammingLds), s, p);
        if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(hamming_merge_kernel, dim3((M + 3) / 4), dim3(256), 0, s, lists, counts, M, N > 0 ? ns : 0, k,
                       out_dist, out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

int cx_rescore_topk(const uint16_t* Q, const uint16_t* D, const int64_t* cand, const int64_t* ids, int M, long R, int d,
                    long ldq, long ldd, int c, int k, const float* below, float* out_scores, int64_t* out_ids,
                    void* stream) {
    if (M < 0 || R < 0 || c < 1 || c > MAXC || k < 1 || k > MAXK || k > c || d < 64 || d > 1024 || (d % 64) != 0)
        return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!Q || !cand || !out_scores || !out_ids || (R > 0 && !D)) return CX_ERR_ARG;
    if (ldq < d || (ldq % 8) != 0 || (R > 0 && (ldd < d || (ldd % 8) != 0))) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)D & 15)) return CX_ERR_ALIGN;
    hipLaunchKernelGGL(rescore_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, Q, D, cand, ids, R, d, ldq, ldd, c, k,
                       below, out_scores, out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

}  // extern "C"
