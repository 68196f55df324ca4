"""The launches of ONE kernel inside a step, each position averaged over the traced steps, from a rocprofv3 rocpd database
(kernel-trace): rocpd_stats.py's average hides that the five proj_kernel<160,256> launches of the c3 step are two short-K and
three long-K ones.  python tools/rocpd_launches.py <results.db> <kernel name substring> <launches per step> [steps to skip = 3]"""
import sqlite3, sys
con = sqlite3.connect(sys.argv[1])
sub, per = sys.argv[2], int(sys.argv[3])
skip = int(sys.argv[4]) if len(sys.argv) > 4 else 3
cur = con.cursor()
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
kt = [t for t in tabs if t.startswith('rocpd_kernel_dispatch')][0]
ks = [t for t in tabs if t.startswith('rocpd_info_kernel_symbol')][0]
cols = [r[1] for r in cur.execute(f"pragma table_info({ks})")]
name = 'display_name' if 'display_name' in cols else ('kernel_name' if 'kernel_name' in cols else cols[-1])
rows = cur.execute(f"select d.start, d.end, s.{name} from {kt} d join {ks} s on d.kernel_id=s.id order by d.start").fetchall()
d = [(e - s) / 1e3 for s, e, n in rows if sub in n]
if not d or len(d) % per:
    sys.exit("%d launches of '%s': no multiple of %d" % (len(d), sub, per))
steps = [d[i:i + per] for i in range(0, len(d), per)][skip:]
print("%s: the %d launches of a step in launch order, us: mean (min .. max) over %d steps" % (sub, per, len(steps)))
for j in range(per):
    v = [s[j] for s in steps]
    print("  launch %d: %6.2f (%6.2f .. %6.2f)" % (j, sum(v) / len(v), min(v), max(v)))
print("  sum     : %6.2f" % (sum(sum(s) for s in steps) / len(steps)))
