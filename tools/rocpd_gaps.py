"""What follows each launch in a rocprofv3 --kernel-trace rocpd database, per kernel name: launches, median duration, median gap
to the start of the NEXT launch (end -> start) and median start-to-start distance.  A producer that writes its dirty lines back
behind its last wave shows that time in the gap, one that writes through shows it in its duration: judge by start-to-start.
Usage: rocpd_gaps.py <db> [name filter regex]   (launches of the whole run; the eager steps at the end of a bench run included)"""
import re
import sqlite3
import statistics
import sys


def main():
    db = sqlite3.connect(sys.argv[1])
    filt = re.compile(sys.argv[2] if len(sys.argv) > 2 else '.')
    rows = list(db.execute('select name, start, end from kernels order by start'))
    per = {}
    for (name, st, en), nxt in zip(rows, rows[1:]):
        if nxt[1] - en > 50000:   # (a host-side pause, not a boundary)
            continue
        short = re.sub(r'\(.*', '', name)
        per.setdefault(short, []).append(((en - st) / 1e3, (nxt[1] - en) / 1e3, (nxt[1] - st) / 1e3, re.sub(r'\(.*', '', nxt[0])))
    print(f'{"kernel":<50} {"n":>5} {"dur_us":>8} {"gap_us":>7} {"s2s_us":>8}  next')
    for name, v in sorted(per.items(), key=lambda kv: -sum(x[2] for x in kv[1])):
        if not filt.search(name):
            continue
        nxt = statistics.mode(x[3] for x in v)
        print(f'{name[:50]:<50} {len(v):5d} {statistics.median(x[0] for x in v):8.2f} {statistics.median(x[1] for x in v):7.2f} '
              f'{statistics.median(x[2] for x in v):8.2f}  {nxt[:40]}')


if __name__ == '__main__':
    main()
