"""What a `rocprofv3 --kernel-trace` CSV says about the launches of a run, without their times: per kernel name the number of dispatches and
the sequence of grid sizes (in dispatch order, run-length encoded), then per queue the order of the names.  Two builds that enqueue the same
launches on the same streams print the same text.

  python3 tools/launch_summary.py <kernel_trace.csv>"""
import csv
import sys


def short(name):
    return name.replace("void ", "").replace("ilqr::", "").split("(")[0]


def rle(seq):
    out = []
    for v in seq:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return " ".join("%s" % v if n == 1 else "%sx%d" % (v, n) for v, n in out)


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    names = sorted({short(r["Kernel_Name"]) for r in rows})
    index = {n: i for i, n in enumerate(names)}
    print("# %d dispatches, %d kernel names" % (len(rows), len(names)))
    for n in names:
        mine = [r for r in rows if short(r["Kernel_Name"]) == n]
        grids = ["%sx%sx%s" % (r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]) if (r["Grid_Size_Y"], r["Grid_Size_Z"]) != ("1", "1") else r["Grid_Size_X"] for r in mine]
        print("[%d] %s: %d dispatches, grids %s" % (index[n], n, len(mine), rle(grids)))
    if rows and "Queue_Id" in rows[0]:
        # queue ids are handles of the run: numbered here in the order of their first dispatch
        queues = []
        for r in rows:
            if r["Queue_Id"] not in queues:
                queues.append(r["Queue_Id"])
        for q, qid in enumerate(queues):
            print("queue %d: %s" % (q, rle([index[short(r["Kernel_Name"])] for r in rows if r["Queue_Id"] == qid])))


if __name__ == "__main__":
    main()
