#!/usr/bin/env python3
"""Which kernel instantiations of the library did a run launch?  Reads the kernel names of one or more rocprofv3 outputs (kernel trace only:
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 -m pytest ...`; every *kernel_stats.csv under DIR is read, one per traced
process) and the launch stubs of the library (nm -C), and prints per kernel family: instantiations in the binary, launched, never launched.
    python3 scripts/kernel_coverage.py DIR [DIR ...] [--matchers] [--lib PATH]
--matchers: only the SGM / block-matching families of tests/matcher_cases.py, and exit 1 if one of their instantiations was never launched."""
import csv
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from matcher_cases import MATCHER_FAMILIES                # noqa: E402

NAME = re.compile(r"(?:\(anonymous namespace\)::|\w+::)*(\w+(?:<[^>]*>)?)\(")


def in_binary(lib):
    out = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", out))


def launched(dirs):
    names, files = {}, []
    for d in dirs:
        files += [d] if os.path.isfile(d) else glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    for f in files:
        for row in csv.DictReader(open(f)):
            m = NAME.search(re.sub(r"^void ", "", row["Name"]))
            if m:
                names[m.group(1)] = names.get(m.group(1), 0) + int(row["Calls"])
    return names, files


def main(argv):
    only = "--matchers" in argv
    lib = argv[argv.index("--lib") + 1] if "--lib" in argv else os.path.join(ROOT, "jackal_navigation_amd", "libjn_stereo.so")
    dirs = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--lib")]
    binary = in_binary(lib)
    calls, files = launched(dirs)
    if not files:
        print("no *kernel_stats.csv under %s" % dirs)
        return 2
    families = {}
    for k in binary:
        families.setdefault(k.split("<")[0], set()).add(k)
    print("# %d kernel instantiations in %s; %d stats file(s) read" % (len(binary), os.path.relpath(lib, ROOT), len(files)))
    missing = 0
    for fam in sorted(families):
        if only and fam not in MATCHER_FAMILIES:
            continue
        inst = families[fam]
        never = sorted(k for k in inst if k not in calls)
        print("%-24s in the binary %3d   launched %3d   never launched %3d%s" % (fam, len(inst), len(inst) - len(never), len(never), "".join("\n    never: " + k for k in never)))
        missing += len(never)
    print("# never launched: %d" % missing)
    return 1 if only and missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
