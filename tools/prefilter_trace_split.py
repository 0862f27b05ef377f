"""Where a pre-filtered pipelined step goes, from a rocprofv3 rocpd database (kernel trace of a bench run):
per-launch time of q8_filter_kernel and of the pre-phase launches (sampling scan_kernel per grid, merge_query_kernel per grid, the
int8 sample's filter / bucket / select), the idle time between one main filter's end and the next one's start, the step (start to
start of consecutive main filters) and how far the pre-phase's last launch ends behind the previous main filter.
    python tools/prefilter_trace_split.py results.db [main-filter launches from the end to use, default 40]"""
import re
import sqlite3
import statistics as st
import sys

db = sqlite3.connect(sys.argv[1])
cur = db.cursor()
last = int(sys.argv[2]) if len(sys.argv) > 2 else 40
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
scols = [r[1] for r in cur.execute(f"pragma table_info({ks})")]
namecol = "display_name" if "display_name" in scols else ("kernel_name" if "kernel_name" in scols else scols[-1])
rows = cur.execute(f"select d.start, d.end, d.grid_size_x, d.workgroup_size_x, s.{namecol} from {kd} d join {ks} s on d.kernel_id = s.id order by d.start").fetchall()
rows = [(a, b, gx // max(wx, 1), re.sub(r"\s+", " ", str(n))) for a, b, gx, wx, n in rows]
filt = [r for r in rows if "q8_filter_kernel" in r[3]]
if not filt:
    sys.exit("no q8_filter_kernel launch in the trace")
main_grid = max(r[2] for r in filt)
mains = [r for r in filt if r[2] == main_grid][-last:]
t_lo, t_hi = mains[0][0], mains[-1][1]
window = [r for r in rows if r[0] >= t_lo and r[1] <= t_hi]


def line(tag, xs):
    if xs:
        print(f"{tag:58s} n {len(xs):4d}  avg {st.mean(xs):8.1f}  median {st.median(xs):8.1f}  min {min(xs):8.1f}  max {max(xs):8.1f}  us")


print(f"window: the last {len(mains)} main filter launches (grid {main_grid}), {(t_hi - t_lo) / 1e6:.2f} ms")
groups = {}
for a, b, g, n in window:
    short = re.sub(r"\(anonymous namespace\)::|^void ", "", n)
    short = re.sub(r"\(.*", "", short)[:40]
    groups.setdefault((short, g), []).append((b - a) / 1e3)
for (short, g), xs in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
    line(f"{short} [grid {g}]", xs)
step = [(mains[i + 1][0] - mains[i][0]) / 1e3 for i in range(len(mains) - 1)]
gap = [(mains[i + 1][0] - mains[i][1]) / 1e3 for i in range(len(mains) - 1)]
line("step: main filter start -> next main filter start", step)
line("gap: main filter end -> next main filter start", gap)
# the sampling launch (bf16 scan_kernel, or the int8 sample's filter) that ends last in front of each main filter: how long it
# ran on behind the PREVIOUS main filter's end (<= 0: hidden under it; its merge / bucket + select follow it)
over = []
for i in range(1, len(mains)):
    pre = [r for r in window if mains[i - 1][0] < r[1] <= mains[i][0] and ("scan_kernel" in r[3] or ("q8_filter_kernel" in r[3] and r[2] != main_grid))]
    if pre:
        over.append((max(r[1] for r in pre) - mains[i - 1][1]) / 1e3)
line("last sampling launch end - previous main filter end", over)
