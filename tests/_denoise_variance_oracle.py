"""rl_denoise_unit_denoise_variance on the CPU: the arithmetic of include/robigo_luculenta.h's variance-guided denoise block in numpy
float32 / float64, one array operation per stated operation, every pixel's taps accumulated in the stated order (dy outer, dx
inner).  rl_expf and the guide record are tests/_denoise_oracle.py's.  Images are (h, w, 3) float32, variances and the error unit's
planes (h, w).  Test-only."""
import numpy as np

from _denoise_oracle import ITERATIONS, TAPS, expf, guide_record, k_of

DEFAULTS = dict(iterations=5, sigma_colour=3.0, sigma_normal=0.3, sigma_depth=0.1, sigma_albedo=0.2)
f32, f64 = np.float32, np.float64


def variance_0(S, Q, k, N):
    """V_0, (h, w) float32, from the error unit's planes S and Q (float64), its observations k and paths N."""
    S, Q = np.asarray(S, np.float64), np.asarray(Q, np.float64)
    n = f64(int(N))                                     # (double)N: Python rounds an int to nearest even, as the conversion does
    with np.errstate(all="ignore"):
        d = Q - (S * S) / n
        d = np.where(d < 0, f64(0), d)                  # (a NaN compares false and stays)
        v = d * (n / f64(int(k) - 1))
        return v.astype(np.float32)


def one_pass(C, V, n, z, a, live, i, kv, kn, kz, ka):
    """(C_{i+1}, V_{i+1}) from (C_i, V_i)."""
    h, w = live.shape
    s = 1 << i
    sum_w = np.zeros((h, w), np.float32)
    sum_c = np.zeros((h, w, 3), np.float32)
    sum_v = np.zeros((h, w), np.float32)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                taken = inside & live[qy, qx] & live
                Cq, Vq, nq, zq, aq = C[qy, qx], V[qy, qx], n[qy, qx], z[qy, qx], a[qy, qx]
                dl = C[..., 1] - Cq[..., 1]
                m = V + Vq
                e_c = np.where(m > 0, (dl * dl) / m, f32(0))
                d = n - nq
                e_n = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                mz = np.where(z > zq, z, zq)
                rz = np.where(mz > 0, (z - zq) / mz, f32(0))
                e_z = rz * rz
                da = a - aq
                e_a = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                x = ((e_c * f32(kv) + e_n * f32(kn)) + e_z * f32(kz)) + e_a * f32(ka)
                wt = (TAPS[dy + 2] * TAPS[dx + 2]) * expf(-x)
                sum_w = np.where(taken, sum_w + wt, sum_w)
                sum_c = np.where(taken[..., None], sum_c + wt[..., None] * Cq, sum_c)
                sum_v = np.where(taken, sum_v + (wt * wt) * Vq, sum_v)
        C1 = np.where(live[..., None], sum_c / sum_w[..., None], C)
        V1 = np.where(live, sum_v / (sum_w * sum_w), V)
    return C1.astype(np.float32), V1.astype(np.float32)


def denoise_v(image, V0, albedo=None, normal=None, aux=None, iterations=0, sigma_colour=3.0, sigma_normal=0.3, sigma_depth=0.1,
              sigma_albedo=0.2, passes=None):
    """(C_iterations, V_iterations) from an (h, w, 3) image and its (h, w) float32 variance V_0; `passes`, a list, receives
    (C_1, V_1), (C_2, V_2), ..."""
    C = np.ascontiguousarray(image, np.float32)
    h, w = C.shape[:2]
    V = np.ascontiguousarray(V0, np.float32).reshape(h, w)
    n, z, a, live = guide_record(albedo, normal, aux, h, w)
    kv, kn, kz, ka = k_of(sigma_colour), k_of(sigma_normal), k_of(sigma_depth), k_of(sigma_albedo)
    for i in range(iterations or ITERATIONS):
        C, V = one_pass(C, V, n, z, a, live, i, kv, kn, kz, ka)
        if passes is not None:
            passes.append((C, V))
    return C, V


def denoise(image, S, Q, k, N, **kw):
    """The call itself: (C, V) for an image and an error unit's state."""
    return denoise_v(image, variance_0(S, Q, k, N), **kw)
