"""Development: the per-kernel split of the burst list's phases from a kernel trace of scripts/bench_bursts.py:
    rocprofv3 --kernel-trace --stats -d DIR -o split -- python scripts/bench_bursts.py 31 LOG
    python scripts/bursts_split.py DIR/split_results.db > profiles/rNN/bursts_kernel_split.log
One line per k_bursts_* kernel and grid size (in lanes): launches, total and mean microseconds.  All legs of the script are in the trace,
so a mean mixes the three threshold legs and both chains; a grid of 256 lanes is one workgroup."""
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
rows = db.execute("""select s.kernel_name, d.grid_size_x, count(*), sum(d.end - d.start) / 1e3, avg(d.end - d.start) / 1e3
                     from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id
                     where s.kernel_name like '%k_bursts%' group by s.kernel_name, d.grid_size_x order by 1, 2""").fetchall()
print("# kernel, grid (lanes), launches, total us, mean us")
for name, grid, n, total, mean in rows:
    short = name[name.index("k_bursts"):].replace("ILi0EEEv", "<COUNT>").replace("ILi1EEEv", "<EMIT>").replace("ENS_", "NS_").split("NS_")[0]
    print(f"{short:24s} {grid:8d} {n:6d} {total:12.1f} {mean:9.2f}")
