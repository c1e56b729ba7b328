// rl_wavelength.h -- wavelength importance sampling: the table of rl_wavelength_table_create and what a path makes of it.  The rule
// is stated in include/robigo_luculenta.h; this is its one implementation.  The table rule is host code, f64 in the stated order --
// add, subtract, multiply, the correctly rounded divide and the f64 -> f32 conversion only -- so the numpy restatement
// (tests/_wavelength_oracle.py) is held bit for bit.  The per-path part is RL_HD, f32, never contracted: the trace kernel's WL
// instantiations (rl_kernels.hip.h) and tests/wavelength_host, the g++ compile for the tests that run without a GPU, read the same text.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "rl_cie1931.h"
#include "rl_core.h"

#define RL_WAVELENGTH_BINS 256        // M
#define RL_WAVELENGTH_MAX_NODES 4096u
// The table as the device reads it: M + 1 quantiles Q, then M weights W -- 513 floats, 2,052 bytes.
#define RL_WAVELENGTH_TABLE_FLOATS (2 * RL_WAVELENGTH_BINS + 1)

enum { RL_WAVELENGTH_OK = 0, RL_WAVELENGTH_OVERFLOW = 1, RL_WAVELENGTH_NOT_INCREASING = 2 };

// An importance that is NaN, infinite or <= 0 counts as 0.
inline double rl_wavelength_importance(double g) { return (g > 0.0 && g < INFINITY) ? g : 0.0; }

// x-bar + y-bar + z-bar of rl_cie1931.h at its 81 nodes (380, 385, ... 780 nm), summed in f64 in that order.
inline void rl_wavelength_cie_importance(double* out) {
    for (int k = 0; k < RL_CIE_SAMPLES; ++k)
        out[k] = ((double)RL_CIE1931_XYZ0[4 * k + 0] + (double)RL_CIE1931_XYZ0[4 * k + 1]) + (double)RL_CIE1931_XYZ0[4 * k + 2];
}

// table: RL_WAVELENGTH_TABLE_FLOATS floats.  importance: n_nodes values at equally spaced wavelengths from 380 to 780 nm inclusive,
// or null for the uniform density.  2 <= n_nodes <= RL_WAVELENGTH_MAX_NODES and 0 < uniform_share <= 1 are the caller's to check.
// On a refusal the table's content is unspecified.
inline int rl_wavelength_table_rule(const double* importance, uint32_t n_nodes, double uniform_share, float* table) {
    const uint32_t n = n_nodes, M = RL_WAVELENGTH_BINS;
    const double nm1 = (double)(n - 1u);
    std::vector<double> d(n - 1u), c(n);
    double g_sum = 0.0;
    if (importance)
        for (uint32_t j = 0; j + 1u < n; ++j) {
            d[j] = (rl_wavelength_importance(importance[j]) + rl_wavelength_importance(importance[j + 1u])) * 0.5; // m_j, for now
            g_sum = g_sum + d[j];
        }
    if (!(g_sum < INFINITY)) return RL_WAVELENGTH_OVERFLOW;
    const bool guided = importance && g_sum > 0.0;
    c[0] = 0.0;
    for (uint32_t j = 0; j + 1u < n; ++j) {
        d[j] = guided ? uniform_share / nm1 + (1.0 - uniform_share) * (d[j] / g_sum) : 1.0 / nm1;
        c[j + 1u] = c[j] + d[j];
    }
    float* q = table;
    float* w = table + (M + 1u);
    const double step = 400.0 / nm1;
    uint32_t j = 0;
    for (uint32_t i = 0; i <= M; ++i) {
        const double t = ((double)i / (double)M) * c[n - 1u];
        while (j + 2u < n && c[j + 1u] <= t) ++j; // the largest j <= n - 2 with C_j <= T_i (T_i does not decrease with i)
        const double lambda = 380.0 + step * ((double)j + (t - c[j]) / d[j]);
        q[i] = (float)lambda;
    }
    q[0] = 380.0f;
    q[M] = 780.0f;
    for (uint32_t i = 0; i < M; ++i)
        if (!(q[i] < q[i + 1u])) return RL_WAVELENGTH_NOT_INCREASING;
    for (uint32_t i = 0; i < M; ++i) w[i] = (float)((((double)q[i + 1u] - (double)q[i]) * (double)M) / 400.0);
    return RL_WAVELENGTH_OK;
}

// ---- per path (RL_HD) ----------------------------------------------------------------------------------------------------------

// The wavelength of a path whose block 0 begins with the word w0: the 24 bits rl_closed01 reads pick a bin (the top 8) and a
// place in it (the other 16).
RL_HD float rl_wavelength_draw(const float* table, uint32_t w0) {
    const uint32_t v = w0 >> 8;
    const uint32_t i = v >> 16;
    const float f = (float)(v & 0xffffu) * 1.52587890625e-5f; // 2^-16
    const float q0 = table[i], q1 = table[i + 1u];
    return q0 + (q1 - q0) * f;
}

// The largest i <= M - 1 with Q[i] <= wavelength: eight steps, no branch (Q[0] = 380 is below every wavelength drawn).
RL_HD uint32_t rl_wavelength_bin(const float* table, float wavelength) {
    uint32_t i = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t step = RL_WAVELENGTH_BINS / 2; step != 0u; step >>= 1)
        i += table[i + step] <= wavelength ? step : 0u;
    return i;
}

// The weight a path of this wavelength carries: a function of the wavelength alone, so a record that restates the draw and a
// splat that kept only the wavelength find the same one.
RL_HD float rl_wavelength_weight(const float* table, float wavelength) {
    return table[RL_WAVELENGTH_BINS + 1u + rl_wavelength_bin(table, wavelength)];
}

// rl_begin_path with the wavelength drawn from the table: every other draw, and everything made of them, word for word.
RL_HD void rl_begin_path_wl(const RlSceneView& sv, float aspect_ratio, uint64_t seed, uint32_t stream, uint64_t path, const float* table,
                            RlPath* p) {
    const RlRngBlock b0 = rl_rng_block(seed, stream, path, 0);
    const float wavelength = rl_wavelength_draw(table, b0.w[0]);
    const float x = rl_get_bi_unit(b0.w[1]);
    const float y = rl_get_bi_unit(b0.w[2]) / aspect_ratio;
    const float t = rl_get_unit(b0.w[3]);
    rl_camera_path(sv, x, y, t, wavelength, seed, stream, path, p);
}
