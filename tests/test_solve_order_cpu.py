"""csrc/solve_order.h: resolve_solve_order, rolls_aside and iteration_order, printed by tests/cpp/solve_order_dump.cpp (host-only C++17, no HIP),
against the rules restated here from the comments of the header, one rule per line.  No GPU.

The cross product of every switch, presence flag, plan and size is ~5e9 combinations; the dump prints four blocks instead, each the full cross
product of some inputs around two bases -- the benchmark's headline (fixed iterations, whole batch, every buffer) and the same with the
convergence exit -- 398 656 combinations in all (solve_order_dump.cpp lists the blocks; BLOCKS below counts them).  Every function of the header
is a conjunction of its inputs or their negations, so a wrong or missing term shows in the block that crosses that input with all the others of its
kind.  iteration_order reads nothing but the SolveOrder: it is printed for every distinct (SolveOrder, max_iter, B) of the four blocks."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc")
SEQUENTIAL, TWIN, DUAL = 0, 1, 2                                        # OrderKind
SWITCHES = ("early_exit", "early_exit_gate", "split", "spec", "spec_dual", "spec_lists", "listed_spec", "dedup", "relin", "repass", "analytic_jacobians", "spec_list_max", "slices")
PRESENCE = ("lists", "chg", "chg_f", "kr", "ls_list", "ls_kind", "lgate", "grp_a", "stream_a", "adopt_events", "twin")
PLAN = ("L.spec_dual", "L.lin_lists", "L.two_lane_line_search", "L.reroll_aside", "L.cold_start_aside")
SIZES = ("B", "max_iter", "spec_list_from")
# block: (rows, the inputs whose combinations it crosses)
BLOCKS = {0: (2 ** 13 * 13, SWITCHES + PRESENCE),                       # (presence: all, none, each one absent)
          1: (2 * 32, ("early_exit", "split", "overlap_rollout", "reuse_rollout", "first_aside", "L.reroll_aside", "L.cold_start_aside")),
          2: (4 * 2 ** 11 * 32, ("early_exit", "split") + PRESENCE + PLAN),
          3: (4 * 3 * 3 * 32 * 2 * 13, SIZES + PLAN + SWITCHES)}
INPUTS = SWITCHES + PRESENCE + PLAN + SIZES + ("spec_max", "overlap_rollout", "reuse_rollout", "first_aside")


def read_table(buf, pos, name):
    end = buf.index(b"\n", pos)
    head = buf[pos:end].decode().split()
    assert head[0] == name
    rows, cols = int(head[1]), head[2:]
    data = np.frombuffer(buf, dtype=np.int16, count=rows * len(cols), offset=end + 1).reshape(rows, len(cols)).astype(np.int64)
    return {c: data[:, i] for i, c in enumerate(cols)}, end + 1 + 2 * rows * len(cols)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("solve_order") / "solve_order_dump")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "solve_order_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 0, r.stderr
    res, pos = read_table(r.stdout, 0, "resolve")
    it, pos = read_table(r.stdout, pos, "iteration")
    assert pos == len(r.stdout)
    return res, it


def expected_order(d):
    """the SolveOrder of every row of the resolve table, rule by rule (d: column -> array)"""
    b = lambda k: d[k] != 0
    e = {}
    # without the convergence exit every rollout stays active: no selection
    e["o.sel_active"] = b("early_exit")
    # the host follows the active count only with the convergence exit, on a batch that has lists; ILQR_EE_GATE=0 switches it off
    e["o.gate"] = b("early_exit") & b("lists") & b("early_exit_gate")
    # bit 1 of k_control's early_exit argument
    e["o.dedup_bit"] = 2 * b("dedup")
    # linearisation cache: needs the lists and chg, analytic kernels that take lists; not with ILQR_RELIN=1
    e["o.cache"] = ~b("relin") & b("lists") & b("chg") & b("L.lin_lists")
    e["o.lin_listed"] = b("early_exit") & b("lists")
    # early continuation: group A's flags, stream and the adoption events; analytic Jacobians only
    e["o.can_split"] = b("split") & b("lists") & b("grp_a") & b("adopt_events") & b("stream_a") & b("analytic_jacobians")
    # first-pass skip: the cache's list and its flags; not with ILQR_REPASS=1, nor in the early-continuation split, nor without list-driven kernels
    e["o.skip_first"] = ~b("repass") & b("lists") & b("chg") & b("chg_f") & b("L.lin_lists") & b("L.spec_dual") & ~e["o.can_split"]
    # the retry's line search from its list: two-lane line search, not beside group A's region
    e["o.retry_gated"] = b("lists") & b("L.two_lane_line_search") & ~e["o.can_split"]
    # side by side: a twin, ILQR_SPEC, lists
    e["o.twin_order"] = b("twin") & b("spec") & b("lists")
    # both orders, chosen on the device: only where the host's count is stale (the gate), ILQR_SPEC_DUAL, list-driven kernels
    e["o.dual_order"] = e["o.twin_order"] & b("spec_dual") & e["o.gate"] & b("L.spec_dual")
    e["o.spec_max"] = d["spec_max"]
    # listed order: its switches; fixed iterations, more than one; the whole batch on one stream set; analytic Jacobians; list-driven kernels;
    # the three skips it rests on allowed; no split; a batch above the whole-batch threshold; its buffers
    e["o.listed_wanted"] = (b("spec") & b("spec_lists") & b("listed_spec") & (d["spec_list_max"] > 0) & ~b("early_exit") & (d["slices"] <= 1) & (d["max_iter"] > 1)
                            & b("analytic_jacobians") & b("L.lin_lists") & b("L.spec_dual") & b("dedup") & ~b("relin") & ~b("repass") & ~b("split") & (d["B"] > d["spec_max"])
                            & b("kr") & b("ls_list") & b("ls_kind") & b("lgate"))
    # ... enqueued only with the twin and where the skips are really on
    e["o.listed"] = e["o.listed_wanted"] & b("twin") & e["o.skip_first"] & e["o.cache"] & ~e["o.gate"]
    # ILQR_SPEC_LIST_FROM, else the last two fifths of the iterations, never iteration 0
    e["o.listed_from"] = np.where(d["spec_list_from"] >= 1, d["spec_list_from"], np.maximum(3 * d["max_iter"] // 5, 1))
    # the twin is worth its memory: ILQR_SPEC, whole batch, and a small batch, or the convergence exit with its gate, or the listed order
    e["o.twin_wanted"] = b("spec") & (d["slices"] <= 1) & ((d["B"] <= d["spec_max"]) | (b("early_exit") & b("early_exit_gate")) | e["o.listed_wanted"])
    for k in ("overlap_rollout", "reuse_rollout", "first_aside"):
        e["o." + k] = b(k)
    # the re-rollout beside the linearisation: iterations >= 1 where it reproduces the candidate, iteration 0 on a cold start by the same kernel
    on = b("overlap_rollout") & ~b("reuse_rollout")
    e["rolls_aside0"] = b("first_aside") & b("L.cold_start_aside") & on
    e["rolls_aside1"] = e["rolls_aside2"] = b("L.reroll_aside") & on
    return {k: np.asarray(v).astype(np.int64) for k, v in e.items()}


def expected_iteration(d):
    """kind, first_listed, pair of every row of the iteration table"""
    twin = (d["o.twin_order"] != 0) & (d["pass_bound"] <= d["o.spec_max"])
    dual = ~twin & (d["o.dual_order"] != 0) & (d["pass_bound"] <= 4 * d["o.spec_max"])
    seq = ~twin & ~dual
    # the first pass from the cache's list: behind a sequential iteration of the same solve (k_control has written the flags)
    first = seq & (d["o.skip_first"] != 0) & (d["iter"] > 0) & (d["prev_seq"] != 0)
    pair = first & (d["o.listed"] != 0) & (d["iter"] >= d["o.listed_from"])
    return {"kind": np.where(twin, TWIN, np.where(dual, DUAL, SEQUENTIAL)), "first_listed": first.astype(np.int64), "pair": pair.astype(np.int64)}


def test_every_block_holds_every_combination_once(tables):
    res, it = tables
    assert set(INPUTS) | {"block"} == {k for k in res if not k.startswith("o.") and not k.startswith("rolls_aside")}
    def distinct(cols):
        """the distinct rows of the table whose columns are cols, sorted (one mixed-radix key per row: the values are few)"""
        key = np.zeros(len(cols[0]), dtype=np.int64)
        for c in cols:
            u, inv = np.unique(c, return_inverse=True)
            key = key * len(u) + inv
        return np.unique(np.stack(cols, axis=1)[np.unique(key, return_index=True)[1]], axis=0)

    for block, (rows, crossed) in BLOCKS.items():
        m = res["block"] == block
        assert m.sum() == rows, (block, m.sum())
        assert len(distinct([res[k][m] for k in crossed])) == rows, block                      # the crossed inputs alone tell the rows apart
        assert len(distinct([res[k][m] for k in INPUTS if k not in crossed])) == 1, block      # everything else: the bases' common values
    assert len(res["block"]) == sum(r for r, _ in BLOCKS.values())
    for k in SWITCHES + PRESENCE + PLAN + ("overlap_rollout", "reuse_rollout", "first_aside"):
        assert len(np.unique(res[k])) == 2, k
    assert set(res["B"]) == {1, 512, 513, 4096} and set(res["max_iter"]) == {1, 2, 10} and set(res["spec_list_from"]) == {0, 1, 4} and set(res["spec_max"]) == {512}
    keys = [it[k] for k in it if k not in ("kind", "first_listed", "pair")]
    assert len(distinct(keys)) == len(keys[0])
    # every order the first table resolves is in the second, with every iteration, five bounds and both prev_seq
    orders = distinct([res[k] for k in res if k.startswith("o.")] + [res["max_iter"], res["B"]])
    bounds = [len({512, 513, 2048, 2049, int(B)}) for B in orders[:, -1]]
    assert len(keys[0]) == 2 * int((orders[:, -2] * bounds).sum())
    assert np.array_equal(distinct([it[k] for k in it if k.startswith("o.")] + [it["max_iter"], it["B"]]), orders)


def test_solve_order_equals_the_rules_in_every_combination(tables):
    res, _ = tables
    e = expected_order(res)
    assert set(e) == {k for k in res if k.startswith("o.") or k.startswith("rolls_aside")}      # every field of the dump is compared
    for k, want in e.items():
        bad = np.flatnonzero(res[k] != want)
        assert len(bad) == 0, (k, len(bad), {c: int(res[c][bad[0]]) for c in res})


def test_iteration_order_equals_the_rules_in_every_combination(tables):
    _, it = tables
    for k, want in expected_iteration(it).items():
        bad = np.flatnonzero(it[k] != want)
        assert len(bad) == 0, (k, len(bad), {c: int(it[c][bad[0]]) for c in it})
    b, s = it["pass_bound"], it["o.spec_max"]
    assert all(((b == v) | (b == it["B"])).any() for v in (s, s + 1, 4 * s, 4 * s + 1))


# ---- the configurations the GPU tests and the benchmark rest on ----------------------------------------------------------------------
def resolved(tables, block=3, **inputs):
    """the ONE row of the block with the base's values but for `inputs`: (its columns, the iteration rows of its order)"""
    res, it = tables
    want = dict(early_exit=0, early_exit_gate=1, spec=1, spec_dual=1, spec_lists=1, listed_spec=1, dedup=1, relin=0, repass=0, analytic_jacobians=1, spec_list_max=1024, slices=1,
                B=4096, max_iter=10, spec_list_from=0, overlap_rollout=1, reuse_rollout=0, first_aside=1, **{k: 1 for k in PRESENCE + PLAN})
    want.update(inputs)
    want.setdefault("split", want["early_exit"])                         # ILQR_SPLIT unset: on with the convergence exit
    m = res["block"] == block
    for k, v in want.items():
        m = m & (res[k] == v)
    (i,) = np.flatnonzero(m)
    row = {k: int(res[k][i]) for k in res}
    mi = np.ones(len(it["iter"]), dtype=bool)
    for k in list(row):
        if k.startswith("o.") or k in ("max_iter", "B"):
            mi = mi & (it[k] == row[k])
    return row, {k: v[mi] for k, v in it.items()}


def walk(rows, bounds):
    """[(kind, first_listed, pair)] of a solve whose iteration i has pass_bound bounds[i], prev_seq following from the kinds"""
    out, prev = [], 0
    for i, pb in enumerate(bounds):
        (j,) = np.flatnonzero((rows["iter"] == i) & (rows["pass_bound"] == pb) & (rows["prev_seq"] == prev))
        out.append((int(rows["kind"][j]), int(rows["first_listed"][j]), int(rows["pair"][j])))
        prev = int(out[-1][0] == SEQUENTIAL)
    return out


def test_headline_listed_pair_from_iteration_six(tables):
    """B = 4096, 10 fixed iterations: iteration 0 full, 1 - 5 the first pass from its list, 6 - 9 the pair (3 * 10 / 5 = 6)"""
    row, its = resolved(tables)
    assert row["o.cache"] and row["o.skip_first"] and row["o.retry_gated"] and row["o.listed"] and row["o.twin_wanted"] and row["o.listed_from"] == 6
    assert not row["o.gate"] and not row["o.sel_active"] and not row["o.can_split"] and not row["o.dual_order"] and row["o.dedup_bit"] == 2
    assert (row["rolls_aside0"], row["rolls_aside1"]) == (1, 1)
    assert walk(its, [4096] * 10) == [(SEQUENTIAL, 0, 0)] + [(SEQUENTIAL, 1, 0)] * 5 + [(SEQUENTIAL, 1, 1)] * 4
    row, its = resolved(tables, spec_list_from=4)
    assert walk(its, [4096] * 10) == [(SEQUENTIAL, 0, 0)] + [(SEQUENTIAL, 1, 0)] * 3 + [(SEQUENTIAL, 1, 1)] * 6


@pytest.mark.parametrize("B", [1, 512])
def test_small_batch_twin_in_every_iteration(tables, B):
    row, its = resolved(tables, B=B)
    assert row["o.twin_wanted"] and row["o.twin_order"] and not row["o.listed"]
    assert walk(its, [B] * 10) == [(TWIN, 0, 0)] * 10


def test_convergence_exit_with_gate_twin_dual_sequential(tables):
    """the host's count: at most 512 side by side, up to 2048 both orders, above sequential; ILQR_SPLIT=0 also brings the first-pass skip"""
    row, its = resolved(tables, early_exit=1)
    assert row["o.gate"] and row["o.sel_active"] and row["o.lin_listed"] and row["o.can_split"] and row["o.twin_wanted"] and row["o.dual_order"]
    assert not row["o.skip_first"] and not row["o.retry_gated"] and not row["o.listed"]
    assert walk(its, [4096, 4096, 2049, 2048, 513, 512, 512]) == [(SEQUENTIAL, 0, 0)] * 3 + [(DUAL, 0, 0)] * 2 + [(TWIN, 0, 0)] * 2
    row, its = resolved(tables, early_exit=1, split=0)
    assert row["o.skip_first"] and row["o.retry_gated"] and not row["o.can_split"] and not row["o.listed"]
    assert walk(its, [4096, 4096, 2049, 2048, 4096, 512]) == [(SEQUENTIAL, 0, 0), (SEQUENTIAL, 1, 0), (SEQUENTIAL, 1, 0), (DUAL, 0, 0), (SEQUENTIAL, 0, 0), (TWIN, 0, 0)]
    row, its = resolved(tables, early_exit=1, early_exit_gate=0)
    assert not row["o.gate"] and not row["o.dual_order"] and not row["o.twin_wanted"]


@pytest.mark.parametrize("inputs, off", [
    ({"analytic_jacobians": 0, "L.lin_lists": 0}, ("o.cache", "o.skip_first", "o.listed", "o.can_split")),      # forward differences
    ({"relin": 1}, ("o.cache", "o.listed")),                                                                  # ILQR_RELIN=1
    ({"repass": 1}, ("o.skip_first", "o.listed")),                                                            # ILQR_REPASS=1
    ({"dedup": 0}, ("o.dedup_bit", "o.listed")),                                                              # ILQR_DEDUP_RETRY=0
])
def test_switches_that_keep_the_full_pass(tables, inputs, off):
    base, _ = resolved(tables)
    row, its = resolved(tables, **inputs)
    assert all(not row[k] for k in off)
    assert all(row[k] == base[k] for k in base if k.startswith("o.") and k not in off + ("o.listed_wanted", "o.twin_wanted"))
    assert not its["pair"].any() and its["first_listed"].any() == bool(row["o.skip_first"])


def test_batch_slices_have_no_lists_and_run_sequential(tables):
    row, its = resolved(tables, block=0, slices=2, **{k: 0 for k in PRESENCE})
    assert not any(row[k] for k in ("o.cache", "o.skip_first", "o.retry_gated", "o.listed", "o.twin_order", "o.twin_wanted", "o.can_split", "o.gate"))
    assert set(its["kind"]) == {SEQUENTIAL} and not its["first_listed"].any()
