#!/usr/bin/env python3
"""actuator_golden.npz: the torque-noise normals of the resident plant's actuator model (include/ilqr_hip.h ilqr_hip_plant_set_actuator) as
the NumPy restatement of tests/actuator_cases.py draws them -- Philox4x32-10 under the pinned counter / key layout in the blocks 32..41,
Box-Muller pairs, the twentieth normal discarded -- and one run of the chain delay line -> lag -> noise, for the 37 records of
actuator_cases.golden_records (delays 0, 1, 2, 3, 4, 8 substeps; tau of 0, 5, 20 and 80 ms mixed per joint; sigma of 0 up to 2 N m), seed
0x0FEDCBA987654321, stream0 0, intervals 0..5 of three substeps at dt = 0.02, under a synthetic command that changes in every substep.

The restatement is first held to the published Philox4x32-10 known-answer vectors; the file also keeps the 32-bit output words of the first
interval, so a test can tell an integer mismatch (never tolerable) from a libm one.

   python tests/golden/gen_actuator_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import actuator_cases as ac        # noqa: E402
import observation_cases as oc     # noqa: E402


def main():
    for counter, key, want in oc.KNOWN_ANSWERS:
        got = oc.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(w) for w in got] == list(want), (counter, key, [hex(int(w)) for w in got])
    B, seed, i0, count, sub = ac.GOLDEN_B, ac.GOLDEN_SEED, ac.GOLDEN_INTERVAL0, ac.GOLDEN_COUNT, ac.GOLDEN_SUBSTEPS
    rec = ac.golden_records()
    assert set(rec[:, 0]) == set(ac.DELAYS) and set(np.unique(rec[:, 1:20])) == set(ac.TAUS) and rec[:, 20:].min() == 0.0 and rec[:, 20:].max() == 2.0
    z = ac.draws(seed, 0, i0, count, B)
    w0 = ac.words(seed, np.arange(B), [i0])[0]
    beta = ac.blend(rec, ac.GOLDEN_DT / sub)
    commands = ac.synthetic_commands(count * sub, B)
    applied = ac.run_chain(rec, beta, commands, z, sub)
    out = os.path.join(HERE, "actuator_golden.npz")
    np.savez_compressed(out, records=rec, seed=np.uint64(seed), stream0=np.int64(0), interval0=np.int64(i0), count=np.int64(count), substeps=np.int64(sub),
                        dt=np.float64(ac.GOLDEN_DT), z=z, words0=w0.astype(np.uint32), beta=beta, commands=commands, applied=applied)
    print("wrote %s: %d records, %d intervals, largest |z| %.2f, %d bytes" % (out, B, count, np.abs(z).max(), os.path.getsize(out)))


if __name__ == "__main__":
    main()
