"""Print VGPR / spill / occupancy per kernel from hipcc -Rpass-analysis=kernel-resource-usage.

    python tools/kernel_resources.py SOURCE.hip [--mangled]

--mangled prints the mangled symbol instead of the demangled name cut to 100 characters (instantiations of one template
collide there): sorted, one line per kernel, so two commits' reports of a file can be compared with diff — a host-side
refactor must leave every line as it was.  Only the device side is compiled."""
import re
import subprocess
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
mangled = "--mangled" in sys.argv[1:]
src = args[0]
r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-Rpass-analysis=kernel-resource-usage"] + (["-mllvm", "-amdgpu-mfma-vgpr-form=1"] if "attention" in src else []) + ["-c", src, "-o", "/dev/null"], capture_output=True, text=True)
if r.returncode != 0:
    sys.exit(r.stderr)
blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
lines = []
for b in blocks:
    name = b.split("\n")[0].strip().split()[0]
    if mangled:
        dn = name
    else:
        dn = subprocess.run(["/usr/bin/c++filt", name], capture_output=True, text=True).stdout.strip()
        dn = re.sub(r"\(.*", "", dn)[:100]

    def g(k):
        m = re.search(k + r": (\d+)", b)
        return int(m.group(1)) if m else -1

    lines.append("%-102s vgpr=%d agpr=%d spill=%d scratch=%d occ=%d lds=%d" % (
        dn, g("VGPRs"), g("AGPRs"), g(r"VGPRs? Spill"), g(r"ScratchSize \[bytes/lane\]"),
        g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")))
print("\n".join(sorted(lines) if mangled else lines))
