// score_tile.h -- the 128 x 128 MFMA score tile of the kernels that walk (query tile x corpus split) without keeping
// candidates: rank.hip (the rank of target columns), range.hip (every column above a per-row bound) and kmeans.hip (the arg-max
// over a centroid table, walked whole by one workgroup).
//
// Scores have search.hip's instruction sequence: v_mfma_f32_16x16x32_bf16 with A := document rows, B := query rows, K
// ascending in 32-wide steps from a zero fp32 accumulator.  An output element of that instruction depends on its own A row
// and B row only, so a pair's score has ONE value whatever tile it is computed in -- the property cx_rescore_topk,
// cx_rank_targets and cx_range_* rest on.  (search.hip keeps its own copy of the loop: it is fused with its selection.)
#pragma once
#include "cx_common.h"

namespace {

constexpr int TM = 128, TN = 128, BK = 64;
constexpr int PANEL = TM * BK * 2;   // 16 KiB: one operand's 64-wide K chunk, 128 rows x 128 B
constexpr int MAXSPLIT = 64;
constexpr long MAX_N = 0x7fffffffL - TN;   // int column indices of the last tile (as search.hip)
constexpr int SPLIT_TARGET_WG = 512;

// [128 rows][8 chunks of 16 B]: chunk c of row r at r*128 + ((c ^ (r & 7)) << 4)  (search.hip's layout)
CX_DEVICE int poff(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// search.hip's tile: acc[a][b][r] = score(query row qrow(a), document row drow(b, r)) of the 128 x 128 tile whose query rows
// start at element offsets qo[i] and document rows at do_[i] (i: this thread's four staging rows tid/8 + 32 i).
// With wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4:
//   qrow(a) = wq*64 + a*16 + l15,   drow(b, r) = wd*64 + b*16 + 4*lh + r.
// ops: 4 * PANEL bytes of LDS (two operands, double-buffered); every barrier of the K loop is inside.
CX_DEVICE void tile_scores(const bf16_t* Q, const bf16_t* D, const int64_t (&qo)[4], const int64_t (&do_)[4], int nk, char* ops,
                           int tid, f32x4_t (&acc)[4][4]) {
    const int lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int c8 = (tid & 7) * 8;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    uint4 sq[4], sd[4];
    auto stage = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sq[i] = *reinterpret_cast<const uint4*>(Q + qo[i] + k0 + c8);
            sd[i] = *reinterpret_cast<const uint4*>(D + do_[i] + k0 + c8);
        }
    };
    auto commit = [&](char* qbuf, char* dbuf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (tid >> 3) + 32 * i, c = tid & 7;
            *reinterpret_cast<uint4*>(qbuf + poff(r, c)) = sq[i];
            *reinterpret_cast<uint4*>(dbuf + poff(r, c)) = sd[i];
        }
    };
    stage(0);
    commit(ops, ops + PANEL);
    __syncthreads();
    for (int kc = 0; kc < nk; ++kc) {
        const char* qb_ = ops + (kc & 1) * 2 * PANEL;
        const char* db_ = qb_ + PANEL;
        stage(min(kc + 1, nk - 1) * BK);   // the last chunk is staged twice, as in search.hip
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t fq[4], fd[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                fq[b] = *reinterpret_cast<const bf16x8_t*>(qb_ + poff(wq * 64 + b * 16 + l15, ks * 4 + lh));
                fd[b] = *reinterpret_cast<const bf16x8_t*>(db_ + poff(wd * 64 + b * 16 + l15, ks * 4 + lh));
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[b], fq[a], acc[a][b], 0, 0, 0);
        }
        char* nq = ops + ((kc + 1) & 1) * 2 * PANEL;   // read last in chunk kc - 1, behind the barrier below
        commit(nq, nq + PANEL);
        __syncthreads();
    }
}

// corpus splits per query tile of a (query tile x corpus split) grid: enough workgroups to fill the chip, at most one per tile
inline int auto_splits(int M, long N, int nsplit) {
    const int tiles_m = (M + TM - 1) / TM;
    const long tiles_n = (N + TN - 1) / TN;
    if (nsplit <= 0) nsplit = (SPLIT_TARGET_WG + tiles_m - 1) / tiles_m;
    nsplit = min(nsplit, MAXSPLIT);
    return (int)max(1L, min((long)nsplit, tiles_n));
}

}  // namespace
