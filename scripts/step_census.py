"""Census of one replayed SAM-BERT step from a rocprofv3 kernel trace of the bench command:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python bench.py --gpus 1 --steps 20 --warmup 5
    python scripts/step_census.py DIR/.../p_kernel_trace.csv > profiles/<tag>_step.txt

Prints, for the last ten steps (a step = the launches between two adam_kernel launches), the number of launches and how many
of them are stock (ATen / rocclr) kernels; then every launch of the last step in start order with hardware queue, start
offset, duration, the gap to the end of everything before it, grid size, a ``*`` for stock kernels and the kernel's name
("Stock launches of the captured step")."""
import collections
import csv
import re
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
print("columns:", list(rows[0].keys()))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
rows.sort(key=lambda r: r["s"])


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n)
    return n[:110]


def stock(n):
    return "at::native" in n or "rocclr" in n or "at::cuda" in n


adam = [i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("adam_kernel")]
print("launches", len(rows), "adam launches", len(adam))
qkey = "Queue_Id" if "Queue_Id" in rows[0] else None
skey = "Stream_Id" if "Stream_Id" in rows[0] else None
# per-step stock counts over the last 10 steps
for a, b in list(zip(adam[:-1], adam[1:]))[-10:]:
    seg = rows[a + 1: b + 1]
    c = sum(1 for r in seg if stock(r["Kernel_Name"]))
    print("step: %d launches, %d stock, %.3f ms first start to last end, %.3f ms kernel time" % (
        len(seg), c, (max(r["e"] for r in seg) - seg[0]["s"]) / 1e6, sum(r["e"] - r["s"] for r in seg) / 1e6))
a, b = adam[-2], adam[-1]
seg = rows[a + 1: b + 1]
t0 = seg[0]["s"]
byq = collections.Counter((r.get(qkey), r.get(skey)) for r in seg)
print("launches per (queue, stream):", dict(byq))
print("stock per (queue, stream):", dict(collections.Counter((r.get(qkey), r.get(skey)) for r in seg if stock(r["Kernel_Name"]))))
names = collections.Counter(short(r["Kernel_Name"])[:70] for r in seg if stock(r["Kernel_Name"]))
for n, c in names.most_common():
    print("  %3d  %s" % (c, n))
print("---- last step, start order: idx queue stream start_us dur_us gap_after_prev_end_us grid name")
prev_end = t0
for i, r in enumerate(seg):
    print("%4d q%s s%s %9.1f %7.1f %6.1f %s %s%s" % (i, r.get(qkey), r.get(skey), (r["s"] - t0) / 1e3, (r["e"] - r["s"]) / 1e3,
                                               (r["s"] - prev_end) / 1e3, r.get("Grid_Size_X", r.get("Grid_Size", "")),
                                               "* " if stock(r["Kernel_Name"]) else "  ", short(r["Kernel_Name"])))
    prev_end = max(prev_end, r["e"])
