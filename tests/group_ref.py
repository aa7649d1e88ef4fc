"""Solve groups (include/ilqr_hip.h ilqr_hip_set_groups) restated in NumPy: the selection rule of ilqr_hip_group_select and the perturbation of
ilqr_hip_group_perturb.  The generator is the Philox4x32-10 restatement of tests/observation_cases.py, which test_observation_cpu.py holds to
the published vectors; the integer part is exact, so the device's draws differ from these by the libm of log / cos / sin alone.

Shared by tests/group_cases.py, tests/test_groups_cpu.py and tests/test_gpu_groups.py."""
import numpy as np

import observation_cases as oc

NU = 19


def select(keys, G):
    """(winner [M] global rollout indices, rec [M, 4]) of keys [M G]: per group the member with the smallest finite key, ties to the lowest
    member, member 0 without a finite key; rec = winner's key, member 0's key, number of finite keys, largest finite key (NaN without)."""
    keys = np.asarray(keys, dtype=np.float64)
    G = int(G)
    assert keys.ndim == 1 and G >= 1 and keys.size % G == 0
    M = keys.size // G
    winner, rec = np.zeros(M, dtype=np.int32), np.zeros((M, 4))
    for m in range(M):
        k = keys[m * G:(m + 1) * G]
        best = 0
        have = bool(np.isfinite(k[0]))
        for g in range(1, G):
            if np.isfinite(k[g]) and (not have or k[g] < k[best]):      # (strictly smaller: among equal keys the lowest member stays)
                best, have = g, True
        fin = k[np.isfinite(k)]
        winner[m] = m * G + best
        rec[m] = (k[best], k[0], fin.size, fin.max() if fin.size else np.nan)
    return winner, rec


def normals(B, count, seed, stream0, draw):
    """z [B, count]: the first `count` standard normals of every rollout's sequence under draw counter `draw` -- block k, counter (stream lo,
    stream hi, draw, k) with stream = stream0 + b and key (seed lo, seed hi), gives the normals 2k and 2k + 1 by Box-Muller"""
    blocks = (int(count) + 1) // 2
    s = (np.uint64(int(stream0) & 0xFFFFFFFFFFFFFFFF) + np.arange(B, dtype=np.uint64))[:, None]
    k = np.arange(blocks, dtype=np.uint64)[None, :]
    s, k = np.broadcast_arrays(s, k)
    counter = np.stack([s & oc.MASK, s >> np.uint64(32), np.full(s.shape, int(draw) & 0xFFFFFFFF, dtype=np.uint64), k], axis=-1)
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    u1, u2 = oc.uniforms(oc.philox4x32_10(counter, np.broadcast_to(key, counter.shape[:-1] + (2,))))
    r = np.sqrt(-2.0 * np.log(u1))
    ang = oc.TWO_PI * u2
    z = np.empty((B, 2 * blocks))
    z[:, 0::2] = r * np.cos(ang)
    z[:, 1::2] = r * np.sin(ang)
    return z[:, :int(count)]


def perturbation(B, N, G, sigma, hold=1, seed=0, stream0=0, draw=0):
    """delta [B, N, 19]: what ilqr_hip_group_perturb adds to ubar under draw counter `draw` -- sigma[row(g)][j] z(b, t // hold, j) for the members
    g = b mod G >= 1, zero for member 0; sigma [1, 19] (row 0 for every member) or [G, 19] (row g)"""
    sigma = np.atleast_2d(np.asarray(sigma, dtype=np.float64))
    assert sigma.shape in ((1, NU), (G, NU)) and hold >= 1 and B % G == 0
    segs = (N + hold - 1) // hold
    z = normals(B, segs * NU, seed, stream0, draw).reshape(B, segs, NU)
    g = np.arange(B) % G
    sig = sigma[np.zeros(B, dtype=np.int64) if sigma.shape[0] == 1 else g]      # [B, 19]
    delta = sig[:, None, :] * z[:, np.arange(N) // hold, :]                       # the product, rounded on its own
    delta[g == 0] = 0.0
    return delta


def perturbed(ubar, G, sigma, hold=1, seed=0, stream0=0, draw=0):
    """ubar [B, N, 19] after one ilqr_hip_group_perturb: the rounded product added; where sigma is zero nothing is added"""
    ubar = np.asarray(ubar, dtype=np.float64)
    B, N, _ = ubar.shape
    return ubar + perturbation(B, N, G, sigma, hold, seed, stream0, draw)
