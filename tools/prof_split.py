"""Per kernel of a rocprofv3 results .db: launches, median us, and the launches below half the median (count, mean us) --
separates the CLS tail's 256-row launches from the full-size launches of the same symbol."""
import re, sqlite3, statistics, subprocess, sys
c = sqlite3.connect(sys.argv[1]); steps = int(sys.argv[2])
tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
ks = [t for t in tabs if "kernel_symbol" in t][0]; kd = [t for t in tabs if "kernel_dispatch" in t][0]
by = {}
for n, d in c.execute(f"select s.kernel_name, d.end-d.start from {kd} d join {ks} s on d.kernel_id=s.id"):
    by.setdefault(n, []).append(d / 1e3)
names = subprocess.run(["c++filt"], input="\n".join(by), capture_output=True, text=True).stdout.split("\n")
print(f"{'kernel':60s} {'n/step':>7s} {'median':>8s} {'large n/step':>12s} {'mean us':>8s} {'small n/step':>12s} {'mean us':>8s}")
for (n, v), dn in sorted(zip(by.items(), names), key=lambda x: -sum(x[0][1])):
    if "vit::" not in dn.split("(")[0]: continue  # (a template kernel demangles with its return type, a plain one without)
    dn = re.sub(r"\(.*", "", dn.replace("void ", "", 1).replace("vit::", "", 1))
    med = statistics.median(v)
    small = [x for x in v if x < med / 2]; large = [x for x in v if x >= med / 2]
    print(f"{dn:60s} {len(v)/steps:7.1f} {med:8.1f} {len(large)/steps:12.1f} {sum(large)/len(large):8.1f} {len(small)/steps:12.1f} {(sum(small)/len(small) if small else 0):8.1f}")
print(f"total kernel time per step: {sum(sum(v) for v in by.values())/steps/1e3:.3f} ms")
