// What the direct-addressed (scn_markov.hip) and the hashed (scn_markov_hash.hip) Markov kernels share: the padded neighbour table, the
// integer behind a Philox draw and the smoothed quotient.  One copy, so that the hashed readers without back-off keep the bits of
// their direct-addressed siblings.
#pragma once
#include "scn_internal.h"

namespace scn_markov {

struct Graph {
    const int32_t* nbr;    // [n_nodes][d]
    const int32_t* deg;    // [n_nodes]
    int n_nodes, d;
    __device__ __forceinline__ bool has(int v) const { return v >= 0 && v < n_nodes; }
    // the real neighbours of the node v in [0, n_nodes): deg[v] clamped to [0, d]
    __device__ __forceinline__ int live_deg(int v) const {
        const int dv = deg[v];
        return dv < 0 ? 0 : (dv > d ? d : dv);
    }
    // slot of b at a, -1 when (a, b) is no edge or an id lies outside [0, n_nodes) (nothing is read through such an id)
    __device__ __forceinline__ int slot(int a, int b) const {
        if (!has(a) || !has(b)) return -1;
        const int dv = live_deg(a);
        const int32_t* row = nbr + (size_t)a * d;
        for (int j = 0; j < dv; ++j)
            if (row[j] == b) return j;
        return -1;
    }
};

// the 24-bit integer behind sample_uniform(seed, root, sample, hop) (scn_internal.h): the same counter and key layout
__device__ __forceinline__ uint32_t uniform_u24(uint64_t seed, int32_t root, int32_t sample, int32_t hop) {
    const uint32_t ctr[4] = {(uint32_t)root, (uint32_t)sample, (uint32_t)hop, 0u};
    const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    uint32_t out[4];
    scn::philox4x32_10(ctr, key, out);
    return out[0] >> 8;
}

// (c_j + alpha) / (total + alpha deg) with every operation rounded on its own: the compiler may not contract the product into the sum
__device__ __forceinline__ double smoothed_weight(double cj, double alpha, double sum, double dv) {
#pragma clang fp contract(off)
    const double scaled = alpha * dv;
    const double den = sum + scaled;
    return den > 0.0 ? (cj + alpha) / den : 0.0;
}

}  // namespace scn_markov
