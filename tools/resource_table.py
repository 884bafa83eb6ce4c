"""Turn hipcc's `-Rpass-analysis=kernel-resource-usage` remarks (read from the files named, or stdin) into one line per
kernel: demangled name, SGPRs, VGPRs, scratch bytes per lane, occupancy (waves per SIMD), LDS bytes.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -DNDEBUG -Rpass-analysis=kernel-resource-usage -c vit_amd/csrc/layernorm.hip \
        -o /dev/null 2> remarks.txt
    python tools/resource_table.py remarks.txt
"""
import re
import subprocess
import sys


def table(text: str):
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = rows.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    names = list(rows)
    try:
        dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        dem = names
    out = []
    for raw, name in zip(names, dem):
        r = rows[raw]
        short = re.sub(r"^void ", "", name.split("(")[0])
        out.append((short, f"sgpr {r.get('TotalSGPRs', '?'):>3}  vgpr {r.get('VGPRs', '?'):>3}  scratch {r.get('ScratchSize', '?'):>3}  "
                           f"occupancy {r.get('Occupancy', '?')}  lds {r.get('LDS', '?')}"))
    return sorted(out)


if __name__ == "__main__":
    text = "".join(open(p).read() for p in sys.argv[1:]) if len(sys.argv) > 1 else sys.stdin.read()
    for name, line in table(text):
        print(f"{name:<48} {line}")
