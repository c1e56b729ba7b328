// rl_adaptive_plan.h -- the plan of rl_adaptive_unit_plan: how many of a batch's camera samples each 16 x 16 tile of the film gets,
// and the weight its splats carry.  The rule is stated in include/robigo_luculenta.h; this is its one implementation: host code,
// f64 in the stated order, add, multiply, the correctly rounded divide, floor and the f64 -> f32 conversion only, so the numpy
// restatement (tests/_adaptive_oracle.py) is held bit for bit.  Plain C++: rl_api.hip includes it, and tests/adaptive_host compiles
// it with g++ for the tests that run without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#define RL_ADAPTIVE_TILE 16 // RL_ERROR_TILE: the tiles are the error unit's

// A tile's cell in continuous pixel coordinates, as the device reads it.
struct RlAdaptiveCell {
    float x_lo, x_hi, y_lo, y_hi;
};

enum { RL_PLAN_OK = 0, RL_PLAN_OVERFLOW = 1, RL_PLAN_EMPTY_TILE = 2, RL_PLAN_REMAINDER = 3 };

// The cell of tile column (or row) i of an axis of `size` pixels: [max(0, 16 i - 0.5), min(size - 1, 16 i + 15.5)].
inline void rl_adaptive_axis_cell(uint32_t i, uint32_t size, double* lo, double* hi) {
    const double a = 16.0 * (double)i - 0.5, b = 16.0 * (double)i + 15.5, last = (double)size - 1.0;
    *lo = a < 0.0 ? 0.0 : a;
    *hi = b > last ? last : b;
}

// An importance that is NaN, infinite or <= 0 counts as 0.
inline double rl_adaptive_importance(double g) { return (g > 0.0 && g < INFINITY) ? g : 0.0; }

// counts, weights, cells: tiles_y * tiles_x entries in raster order (cells may be null).  width, height >= 2, 0 < uniform_share <= 1
// and 1 <= n_paths <= 2^32 - 1 are the caller's to check.  On any failure nothing the caller holds is a plan: it writes into
// buffers of its own and keeps what it had.
inline int rl_adaptive_plan_rule(uint32_t width, uint32_t height, const double* importance, double uniform_share, uint64_t n_paths,
                                 uint32_t* counts, float* weights, RlAdaptiveCell* cells, double* importance_sum) {
    const uint32_t tiles_x = (width + RL_ADAPTIVE_TILE - 1u) / RL_ADAPTIVE_TILE, tiles_y = (height + RL_ADAPTIVE_TILE - 1u) / RL_ADAPTIVE_TILE;
    const size_t n_tiles = (size_t)tiles_x * tiles_y;
    const double area = ((double)width - 1.0) * ((double)height - 1.0), n = (double)n_paths;
    double g_sum = 0.0;
    if (importance)
        for (size_t t = 0; t < n_tiles; ++t) g_sum = g_sum + rl_adaptive_importance(importance[t]);
    if (importance_sum) *importance_sum = g_sum;
    if (!(g_sum < INFINITY)) return RL_PLAN_OVERFLOW;
    const bool guided = g_sum > 0.0;
    std::vector<double> a(n_tiles), rest(n_tiles);
    std::vector<uint64_t> c(n_tiles);
    uint64_t given = 0;
    for (size_t t = 0; t < n_tiles; ++t) {
        double x_lo, x_hi, y_lo, y_hi;
        rl_adaptive_axis_cell((uint32_t)(t % tiles_x), width, &x_lo, &x_hi);
        rl_adaptive_axis_cell((uint32_t)(t / tiles_x), height, &y_lo, &y_hi);
        if (cells) cells[t] = RlAdaptiveCell{(float)x_lo, (float)x_hi, (float)y_lo, (float)y_hi};
        a[t] = (x_hi - x_lo) * (y_hi - y_lo);
        const double qa = a[t] / area;
        const double q = guided ? uniform_share * qa + (1.0 - uniform_share) * (rl_adaptive_importance(importance[t]) / g_sum) : qa;
        const double e = n * q, f = floor(e);
        c[t] = (uint64_t)f;
        rest[t] = e - f;
        given += c[t];
    }
    // Largest remainder: the paths the floors leave over go one each to the tiles with the largest e - floor(e), ties to the lower
    // tile index.  (The shares sum to 1 within n_tiles rounding errors, so what is left over is an integer of [0, n_tiles].)
    if (given > n_paths || n_paths - given > n_tiles) return RL_PLAN_REMAINDER;
    const size_t left = (size_t)(n_paths - given);
    if (left > 0) {
        std::vector<uint32_t> order(n_tiles);
        for (size_t t = 0; t < n_tiles; ++t) order[t] = (uint32_t)t;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t i, uint32_t j) { return rest[i] > rest[j]; });
        for (size_t k = 0; k < left; ++k) c[order[k]] += 1;
    }
    for (size_t t = 0; t < n_tiles; ++t)
        if (c[t] == 0) return RL_PLAN_EMPTY_TILE;
    for (size_t t = 0; t < n_tiles; ++t) {
        counts[t] = (uint32_t)c[t];
        weights[t] = (float)((n * a[t]) / (area * (double)c[t]));
    }
    return RL_PLAN_OK;
}
