"""min / median / max of single launches' device durations over the forwards of a rocprofv3 kernel trace (rocpd sqlite database) - the
spread a per-launch before / after comparison has to clear (scripts/trace_sequence.py prints the means).

usage: python scripts/trace_launch_stats.py <results.db> <dispatches per forward> <forwards> <launch index> [<launch index> ...]
"""
import sqlite3
import sys


def main(path, nops, nfwd, idx):
    c = sqlite3.connect(path)
    tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if "kernel_dispatch" in t][0]
    ks = [t for t in tabs if "kernel_symbol" in t][0]
    rows = c.execute(f"select d.start, d.end, s.kernel_name from {kd} d join {ks} s on d.kernel_id=s.id order by d.start").fetchall()
    rows = rows[-nops * nfwd:]
    for i in idx:
        d = sorted((rows[f * nops + i][1] - rows[f * nops + i][0]) / 1e3 for f in range(nfwd))
        names = {rows[f * nops + i][2] for f in range(nfwd)}
        assert len(names) == 1, ("launch %d is not the same kernel in every forward" % i, names)
        print("#%d over %d forwards: min %.2f  median %.2f  max %.2f us  (max - min %.2f)  %s"
              % (i, nfwd, d[0], d[len(d) // 2], d[-1], d[-1] - d[0], names.pop().replace("_ZN12saber_mi355x", "")[:70]))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), [int(a) for a in sys.argv[4:]])
