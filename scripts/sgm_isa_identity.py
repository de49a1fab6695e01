#!/usr/bin/env python3
"""Is the device code of csrc/sgm_sweep.hip the same in two source trees?  (no GPU needed)
   python3 scripts/sgm_isa_identity.py <tree A> <tree B>
Compiles the file of both trees for gfx950 to assembly with the Makefile's flags, three times (release, -DJN_HOOKS, -DJN_SGM_PROFILE), and
compares, kernel for kernel with the mangled names blanked, the instruction streams and the resource remarks as MULTISETS (a kernel that was
renamed or moved in the file still pairs with itself).  Exit status 0: identical in all three builds."""
import collections, re, subprocess, sys, tempfile

FLAGS = ["-O3", "-mavx2", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
BUILDS = (("release", []), ("hooks", ["-DJN_HOOKS"]), ("profile", ["-DJN_SGM_PROFILE"]))


def blank(s):
    return re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", re.sub(r"_Z\w+", "_Z", s))


def device_code(tree, extra):
    """(Counter of per-kernel instruction streams, Counter of per-kernel resource remarks, instructions in all)"""
    with tempfile.NamedTemporaryFile(suffix=".s") as out:
        r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + [tree + "/jackal_navigation_amd/csrc/sgm_sweep.hip", "-o", out.name], capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        asm = open(out.name).read().split("\n")
    streams, total, i = collections.Counter(), 0, 0
    while i < len(asm):
        if not re.match(r"^_Z\w+:", asm[i]):
            i += 1
            continue
        body = []
        i += 1
        while not asm[i].startswith(".Lfunc_end"):
            line = blank(asm[i].split(";")[0].rstrip())
            if line and not line.lstrip().startswith("."):        # instructions and labels; directives carry nothing the remarks do not
                body.append(line)
                total += not line.endswith(":")
            i += 1
        streams["\n".join(body)] += 1
    remarks, cur = collections.Counter(), None
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if m and m.group(1).startswith("Function Name:"):
            if cur is not None:
                remarks[tuple(cur)] += 1
            cur = []
        elif m:
            cur.append(m.group(1))
    remarks[tuple(cur)] += 1
    return streams, remarks, total


same = True
for name, extra in BUILDS:
    (sa, ra, ta), (sb, rb, tb) = device_code(sys.argv[1], extra), device_code(sys.argv[2], extra)
    ok = sa == sb and ra == rb
    same &= ok
    print("%-8s A: %d kernels, %d instructions   B: %d kernels, %d instructions   streams %s, resources %s" %
          (name, sum(sa.values()), ta, sum(sb.values()), tb, "equal" if sa == sb else "DIFFER (%d kernels)" % sum((sa - sb).values()),
           "equal" if ra == rb else "DIFFER (%d kernels)" % sum((ra - rb).values())))
sys.exit(0 if same else 1)
