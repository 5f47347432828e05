// ln_workspace.h -- the one rule that decides whether a LayerNorm backward (layernorm.hip) takes its workspace route, shared
// with the callers that must know the answer before they call (engine.hip: a bias gradient rides along as the column sums
// of dz only on that route).
#pragma once

// True when the fp32 workspace holds `n_vec` partial vectors of width d (2: dgamma, dbeta; 3: also the column sums) for
// 256 blocks, one per CU: with fewer the two-stage reduction would launch fewer blocks than the atomics route does.
inline bool cx_ln_bwd_ws_holds(const float* ws, long ws_floats, int n_vec, int d) {
    return ws && ws_floats >= (long)n_vec * d * 256;
}
