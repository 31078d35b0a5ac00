"""Compare the kernels of two device-assembly files (hipcc ... --cuda-device-only -S) of one
source before and after a change: which kernels exist on either side, whether each pair has the
same instruction stream, and the VGPR / SGPR / LDS / scratch figures of both builds.

    python tools/kernel_asm_diff.py old.s new.s [--map OLD_REGEX NEW_TEMPLATE]... [--table]

Names are compared demangled, without the parameter list; --map rewrites an old name (re.sub)
to the name it has in the new file.  Local labels are renumbered per kernel.  A pair that differs
only in the immediate offsets of its kernel-argument loads (s_load_* from the SGPR pair the
kernel's first s_load reads: the kernel-argument segment) is reported as "kernarg offsets only";
different register / LDS / scratch figures count as different.  Exit status 1 if any pair differs
otherwise or a kernel has no partner.
"""
import argparse
import re
import subprocess
import sys

CXXFILT = "c++filt"
RES = {"vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)",
       "lds": r"; LDSByteSize: (\d+)", "scratch": r"; ScratchSize: (\d+)"}


def kernels(path):
    """{demangled name: (body lines, {resource: value})} of every .amdhsa_kernel in the file."""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    plain = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    out = {}
    for sym, name in zip(names, plain):
        start = text.index(f"\n{sym}:") + 1
        end = text.index(".Lfunc_end", start)
        body = []
        labels = {}
        for line in text[start:end].split("\n")[1:]:
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):
                if line.startswith(".LBB") and line.endswith(":"):
                    labels.setdefault(line[:-1], f"L{len(labels)}")
                    body.append(labels[line[:-1]] + ":")
                continue
            body.append(line)
        body = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), b) for b in body]
        tail = text[end:end + 4000]
        name = name.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]  # no parameter list
        out[name] = (body, {k: int(re.search(v, tail).group(1)) for k, v in RES.items()})
    return out


def kernarg_ptr(body):
    """The SGPR pair that the first s_load_* reads from: the kernel-argument segment."""
    for b in body:
        m = re.match(r"s_load_\w+ \S+ (s\[\d+:\d+\]), ", b)
        if m:
            return m.group(1)
    return None


def strip_kernarg_offsets(body):
    base = kernarg_ptr(body)
    if base is None:
        return body
    pat = re.compile(r"(s_load_\w+ \S+ " + re.escape(base) + r"), 0x[0-9a-f]+")
    return [pat.sub(r"\1, OFF", b) for b in body]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", nargs=2, action="append", default=[], metavar=("OLD_REGEX", "NEW_TEMPLATE"))
    ap.add_argument("--table", action="store_true", help="print the per-kernel resource table")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    renamed = {}
    for name in old:
        to = name
        for pat, tmpl in a.map:
            to = re.sub(pat, tmpl, to)
        renamed[to] = name
    counts = {"identical": 0, "kernarg offsets only": 0, "DIFFERENT": 0}
    rows = []
    for name in sorted(set(renamed) | set(new)):
        if name not in new or name not in renamed:
            rows.append((name, "ONLY IN " + ("old" if name in renamed else "new"), None, None))
            counts["DIFFERENT"] += 1
            continue
        (bo, ro), (bn, rn) = old[renamed[name]], new[name]
        if bo == bn:
            verdict = "identical"
        elif strip_kernarg_offsets(bo) == strip_kernarg_offsets(bn):
            verdict = "kernarg offsets only"
        else:
            verdict = "DIFFERENT"
        if ro != rn:
            verdict = "DIFFERENT"
        counts[verdict] += 1
        rows.append((name, verdict, ro, rn))
    print(f"kernels: old {len(old)}, new {len(new)}; " + ", ".join(f"{k}: {v}" for k, v in counts.items()))
    if a.table:
        print("| kernel (new name) | instructions | verdict | VGPR old/new | SGPR old/new | LDS old/new "
              "| scratch old/new |")
        print("|---|---|---|---|---|---|---|")
        for name, verdict, ro, rn in rows:
            if ro is None:
                print(f"| `{name}` | | {verdict} | | | | |")
                continue
            n = sum(not b.endswith(":") for b in new[name][0])
            res = " | ".join(f"{ro[k]}/{rn[k]}" for k in ("vgpr", "sgpr", "lds", "scratch"))
            print(f"| `{name}` | {n} | {verdict} | {res} |")
    return 1 if counts["DIFFERENT"] else 0


if __name__ == "__main__":
    sys.exit(main())
