"""The observation model of the resident plant (include/ilqr_hip.h ilqr_hip_plant_set_observation) restated in NumPy: the Philox4x32-10
generator with the counter / key layout the header pins, the Box-Muller pairs, the state-shaped error row and the composition x [+] delta.
The integer part is exact, so the device's draws differ from these by the libm of log / cos / sin alone.

Shared by tests/test_observation_cpu.py, tests/test_gpu_observation.py and tests/golden/gen_observation_golden.py."""
import os

import numpy as np

NX, NT, REC = 51, 50, 100
BLOCKS = 25
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observation_golden.npz")

# the published Philox4x32-10 vectors (Random123 kat_vectors): counter, key, output
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (32-bit values in any integer type) -> output words [..., 4] as uint64 holding 32-bit values"""
    c = [np.asarray(counter)[..., k].astype(np.uint64) & MASK for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) & MASK for k in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 bits: the product fits 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(*c), axis=-1)


def uniforms(words):
    """output words [..., 4] -> (u1, u2), each ((hi << 32 | lo) >> 11) + 0.5 scaled by 2^-53 in double arithmetic"""
    n1 = ((words[..., 0] << np.uint64(32)) | words[..., 1]) >> np.uint64(11)
    n2 = ((words[..., 2] << np.uint64(32)) | words[..., 3]) >> np.uint64(11)
    return (n1.astype(np.float64) + 0.5) * 2.0 ** -53, (n2.astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, streams, intervals):
    """z [len(intervals), len(streams), 50]: the standard normals of rollout stream s in plant interval i"""
    seed = int(seed)
    s = np.asarray(streams, dtype=np.uint64)[None, :, None]
    i = np.asarray(intervals, dtype=np.uint64)[:, None, None]
    k = np.arange(BLOCKS, dtype=np.uint64)[None, None, :]
    s, i, k = np.broadcast_arrays(s, i, k)
    counter = np.stack([s & MASK, s >> np.uint64(32), i & MASK, k], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    u1, u2 = uniforms(philox4x32_10(counter, np.broadcast_to(key, counter.shape[:-1] + (2,))))
    r = np.sqrt(-2.0 * np.log(u1))
    ang = TWO_PI * u2
    z = np.empty(u1.shape[:-1] + (NT,))
    z[..., 0::2] = r * np.cos(ang)
    z[..., 1::2] = r * np.sin(ang)
    return z


def error_rows(e):
    """tangent errors e [..., 50] -> state-shaped rows delta [..., 51]"""
    e = np.asarray(e, dtype=np.float64)
    d = np.empty(e.shape[:-1] + (NX,))
    d[..., 0:3] = e[..., 0:3]
    w = e[..., 3:6]
    th = np.sqrt(w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2])
    zero = th == 0.0
    safe = np.where(zero, 1.0, th)
    d[..., 3] = np.where(zero, 1.0, np.cos(0.5 * th))
    d[..., 4:7] = np.where(zero, 0.0, np.sin(0.5 * th) / safe)[..., None] * w
    d[..., 7:] = e[..., 6:]
    return d


def errors(records, seed, stream0, interval0, count, B=None):
    """delta [count, B, 51] for records [1 or B, 100] (bias[50], sigma[50]): what ilqr_hip_plant_observation_errors returns"""
    records = np.atleast_2d(np.asarray(records, dtype=np.float64))
    B = records.shape[0] if B is None else int(B)
    rec = np.broadcast_to(records, (B, REC))
    z = normals(seed, int(stream0) + np.arange(B), int(interval0) + np.arange(int(count)))
    sz = rec[None, :, NT:] * z
    return error_rows(rec[None, :, :NT] + sz)


def boxplus(x, d):
    """x [+] delta: positions and everything behind the quaternion added, quat (x) delta.quat (Hamilton, wxyz), not renormalised"""
    x, d = np.asarray(x, dtype=np.float64), np.asarray(d, dtype=np.float64)
    out = x + d
    a, b = x[..., 3:7], d[..., 3:7]
    out[..., 3] = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3]
    out[..., 4] = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2]
    out[..., 5] = a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1]
    out[..., 6] = a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]
    return out


# ---- the records of the golden and of the GPU tests: B = 37 (tests/plant_params_cases.py), |bias| <= 1, 0 <= sigma <= 1
GOLDEN_B, GOLDEN_SEED, GOLDEN_INTERVAL0, GOLDEN_COUNT = 37, 0x1234_5678_9ABC_DEF1, 0, 6


def golden_records(B=GOLDEN_B, seed=11):
    """rollout b % 4: bias and noise / bias alone / noise alone / a zero record; one rollout at the bounds"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((B, REC))
    b = np.arange(B)
    rec[:, :NT] = np.where((b % 4 < 2)[:, None], rng.uniform(-1.0, 1.0, (B, NT)), 0.0)
    rec[:, NT:] = np.where(np.isin(b % 4, (0, 2))[:, None], rng.uniform(0.0, 1.0, (B, NT)), 0.0)
    rec[4, :NT] = np.where(np.arange(NT) % 2 == 0, 1.0, -1.0)
    rec[4, NT:] = 1.0
    return rec


def plant_records(B, seed=5):
    """records a closed loop survives and still feels: centimetres, hundredths of a radian, 0.05 rad/s; rollout b % 3 == 2 sees the truth"""
    rng = np.random.default_rng(seed)
    scale = np.concatenate([np.full(3, 0.01), np.full(3, 0.02), np.full(19, 0.01), np.full(3, 0.05), np.full(3, 0.05), np.full(19, 0.05)])
    rec = np.zeros((B, REC))
    rec[:, :NT] = rng.uniform(-1.0, 1.0, (B, NT)) * scale
    rec[:, NT:] = rng.uniform(0.0, 1.0, (B, NT)) * scale
    rec[np.arange(B) % 3 == 2] = 0.0
    return rec


def golden():
    return np.load(GOLDEN)
