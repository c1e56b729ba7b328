"""rl_denoise_unit_denoise on the CPU: the arithmetic of include/robigo_luculenta.h's denoise block in numpy float32, one array
operation per stated operation, every pixel's taps accumulated in the stated order (dy outer, dx inner).  rl_expf is the oracle
library's (oracle_math_f32(3, ...), as tests/_step_oracle.py calls it); rl_sqrtf is np.sqrt on float32, which is correctly
rounded; float32 +, -, *, / of numpy are the IEEE ones.  Images are (h, w, 3) float32 arrays.  Test-only."""
import numpy as np

import _oracle as O

ITERATIONS, MAX_ITERATIONS = 5, 6
DEFAULTS = dict(iterations=5, sigma_colour=0.6, sigma_normal=0.3, sigma_depth=0.1, sigma_albedo=0.2)
TAPS = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
f32 = np.float32


def expf(x):
    """rl_expf of a float32 array."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    O.lib().oracle_math_f32(3, O.ptr(x), O.ptr(y), x.size)
    return y


def k_of(sigma):
    s = f32(sigma)
    return f32(0) if s == 0 else f32(1) / (s * s)


def guide_record(albedo, normal, aux, h, w):
    """(n (h, w, 3), z (h, w), a (h, w, 3), live (h, w) bool) from the three films, each (h, w, 3) float32 or None."""
    with np.errstate(all="ignore"):
        X = np.asarray(aux, np.float32).reshape(h, w, 3) if aux is not None else np.tile(np.array([1, 0, 0], np.float32), (h, w, 1))
        A = np.asarray(albedo, np.float32).reshape(h, w, 3) if albedo is not None else np.zeros((h, w, 3), np.float32)
        N = np.asarray(normal, np.float32).reshape(h, w, 3) if normal is not None else np.zeros((h, w, 3), np.float32)
        wgt = X[..., 0]
        live = wgt > 0
        z = np.where(live, X[..., 1] / wgt, f32(0))
        a = np.where(live[..., None], A / wgt[..., None], f32(0))
        l2 = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
        length = np.sqrt(l2)
        n = np.where((length > 0)[..., None], N / length[..., None], f32(0))
    return n.astype(np.float32), z.astype(np.float32), a.astype(np.float32), live


def one_pass(C, n, z, a, live, i, kc, kn, kz, ka):
    """C_{i+1} from C_i."""
    h, w = live.shape
    s = 1 << i
    kc_i = f32(kc) * f32(1 << (2 * i))
    sum_w = np.zeros((h, w), np.float32)
    sum_c = np.zeros((h, w, 3), np.float32)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                taken = inside & live[qy, qx] & live
                Cq, nq, zq, aq = C[qy, qx], n[qy, qx], z[qy, qx], a[qy, qx]
                m = np.abs(C[..., 1]) + np.abs(Cq[..., 1])
                r = np.where(m > 0, (C[..., 1] - Cq[..., 1]) / m, f32(0))
                e_c = r * r
                d = n - nq
                e_n = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                mz = np.where(z > zq, z, zq)
                rz = np.where(mz > 0, (z - zq) / mz, f32(0))
                e_z = rz * rz
                da = a - aq
                e_a = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                x = ((e_c * kc_i + e_n * f32(kn)) + e_z * f32(kz)) + e_a * f32(ka)
                wt = (TAPS[dy + 2] * TAPS[dx + 2]) * expf(-x)
                sum_w = np.where(taken, sum_w + wt, sum_w)
                sum_c = np.where(taken[..., None], sum_c + wt[..., None] * Cq, sum_c)
        out = np.where(live[..., None], sum_c / sum_w[..., None], C)
    return out.astype(np.float32)


def denoise(image, albedo=None, normal=None, aux=None, iterations=0, sigma_colour=0.6, sigma_normal=0.3, sigma_depth=0.1, sigma_albedo=0.2,
            passes=None):
    """dst's tristimulus buffer, (h, w, 3) float32, for an (h, w, 3) image; `passes`, a list, receives C_1, C_2, ..."""
    C = np.ascontiguousarray(image, np.float32)
    h, w = C.shape[:2]
    n, z, a, live = guide_record(albedo, normal, aux, h, w)
    kc, kn, kz, ka = k_of(sigma_colour), k_of(sigma_normal), k_of(sigma_depth), k_of(sigma_albedo)
    for i in range(iterations or ITERATIONS):
        C = one_pass(C, n, z, a, live, i, kc, kn, kz, ka)
        if passes is not None:
            passes.append(C)
    return C
