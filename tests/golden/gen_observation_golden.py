#!/usr/bin/env python3
"""observation_golden.npz: the observation errors of the resident plant (include/ilqr_hip.h ilqr_hip_plant_set_observation) as the NumPy
restatement of tests/observation_cases.py draws them -- Philox4x32-10 under the pinned counter / key layout, Box-Muller pairs, the
state-shaped row -- for the 37 records of observation_cases.golden_records (|bias| <= 1, 0 <= sigma <= 1: bias and noise, bias alone, noise
alone, zero records, one record at the bounds), seed 0x123456789ABCDEF1, stream0 0, intervals 0..5.

The restatement is first held to the published Philox4x32-10 known-answer vectors; the file also keeps the 32-bit output words of the first
interval, so a test can tell an integer mismatch (never tolerable) from a libm one.

   python tests/golden/gen_observation_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import observation_cases as oc     # noqa: E402


def main():
    for counter, key, want in oc.KNOWN_ANSWERS:
        got = oc.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(w) for w in got] == list(want), (counter, key, [hex(int(w)) for w in got])
    B, seed, i0, count = oc.GOLDEN_B, oc.GOLDEN_SEED, oc.GOLDEN_INTERVAL0, oc.GOLDEN_COUNT
    rec = oc.golden_records()
    assert np.abs(rec).max() <= 1.0 and rec[:, oc.NT:].min() >= 0.0
    delta = oc.errors(rec, seed, 0, i0, count)
    z = oc.normals(seed, np.arange(B), i0 + np.arange(count))
    s, k = np.broadcast_arrays(np.arange(B, dtype=np.uint64)[:, None], np.arange(oc.BLOCKS, dtype=np.uint64)[None, :])
    counter = np.stack([s, np.zeros_like(s), np.full_like(s, i0), k], axis=-1)
    words = oc.philox4x32_10(counter, np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), counter.shape[:-1] + (2,)))
    out = os.path.join(HERE, "observation_golden.npz")
    np.savez_compressed(out, records=rec, seed=np.uint64(seed), stream0=np.int64(0), interval0=np.int64(i0), count=np.int64(count), delta=delta, z=z,
                        words0=words.astype(np.uint32))
    print("wrote %s: %d records, %d intervals, largest |z| %.2f, %d bytes" % (out, B, count, np.abs(z).max(), os.path.getsize(out)))


if __name__ == "__main__":
    main()
