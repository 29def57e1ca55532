"""Development aid: per-specialisation register / scratch / LDS use from hipcc's -Rpass-analysis=kernel-resource-usage
output (scripts/build_dev.sh writes it to /tmp/shc_res.txt).  Usage: regs.py [report [kernel name]]: the cycle kernels by default, or the
kernels whose name contains `kernel name` (e.g. leg_state_msgs_kernel: legs, dof, VGPR, SGPR, LDS, scratch; footholds_: legs, element type, ...)."""
import re
import sys

t = open(sys.argv[1] if len(sys.argv) > 1 else "/tmp/shc_res.txt").read()
for b in re.split(r"remark: [^\n]*Function Name: ", t)[1:]:
    name = b.split()[0]
    if len(sys.argv) > 2:
        if sys.argv[2] not in name:
            continue
        m = re.search(r"ILi(\d)ELi(\d)E", name)
        g = lambda k: re.search(k + r": (\d+)", b).group(1)
        f = re.search(r"ILi\dELi\dELj(\d+)E(?:Li([012])E)?", name)   # the loop forms: feature word, and the helper wavefronts per robot group of shc_resident2_kernel
        form = ("features %-10s %s" % (f.group(1), {"1": "1 helper ", "2": "2 helpers"}.get(f.group(2), "         ")),) if f else ()
        one = re.search(r"ILi(\d)E([fd])E", name)   # kernels on the leg count and an element type only (footholds_set_kernel / footholds_get_kernel)
        head = "legs %s dof %s" % m.groups() if m else "legs %s %s" % (one.group(1), {"f": "float32", "d": "float64"}[one.group(2)]) if one else "legs ? dof ?"
        print(head, name.split("I")[0][4:], *form, "VGPR", g("VGPRs"), "AGPR", g("AGPRs"), "SGPR", g("TotalSGPRs"),
              "LDS", g(r"LDS Size \[bytes/block\]"), "scratch", g(r"ScratchSize \[bytes/lane\]"), "waves/SIMD", g(r"Occupancy \[waves/SIMD\]"))
        continue
    if "shc_cycle_kernel" not in name:
        continue
    m = re.search(r"ILi(\d)ELi(\d)ELj(\d+)E", name)
    g = lambda k: re.search(k + r": (\d+)", b).group(1)
    print("legs %s dof %s features %-10s" % m.groups(), "VGPR", g("VGPRs"), "AGPR", g("AGPRs"), "scratch", g(r"ScratchSize \[bytes/lane\]"),
          "waves/SIMD", g(r"Occupancy \[waves/SIMD\]"), "LDS", g(r"LDS Size \[bytes/block\]"))
