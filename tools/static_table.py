"""Static table of the kernels of one or two `hipcc -S` device listings: instructions all / VALU / scalar / v_writelane+v_readlane,
then VGPRs / scratch bytes per lane, per kernel whose demangled name matches a filter; with two listings, the first on the left, and a
line at the end that names every kernel with more VGPRs or scratch on the right.
Usage: python tools/static_table.py LEFT.s [RIGHT.s] [--match REGEX]     (listings: hipcc --offload-arch=gfx950 -O3 -std=c++17
-fno-slp-vectorize --offload-device-only -S FILE.hip, plus the file's flags of __graft_entry__.FILE_FLAGS)"""
import re
import subprocess
import sys


def kernels(path):
    """-> {mangled name: dict(all, valu, scalar, lanes, vgpr, scratch, ops)}"""
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name, cur = m.group(1), {"all": 0, "valu": 0, "scalar": 0, "lanes": 0, "ops": {}}
            continue
        if cur is None:
            continue
        s = line.strip()
        if s.startswith(".amdhsa_kernel"):
            continue
        m = re.match(r"^; (NumVgprs|ScratchSize): (\d+)", s)
        if m:
            cur["vgpr" if m.group(1) == "NumVgprs" else "scratch"] = int(m.group(2))
            if "vgpr" in cur and "scratch" in cur:
                out[name] = cur
                cur = None
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        op = s.split()[0]
        cur["all"] += 1
        cur["ops"][op] = cur["ops"].get(op, 0) + 1
        if op in ("v_writelane_b32", "v_readlane_b32"):
            cur["lanes"] += 1
        if op.startswith("v_"):
            cur["valu"] += 1
        elif op.startswith("s_"):
            cur["scalar"] += 1
    return out


def demangle(names):
    text = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", d)) for n, d in zip(names, text)}


def main():
    args = [a for a in sys.argv[1:]]
    pat = re.compile(args[args.index("--match") + 1]) if "--match" in args else re.compile(".")
    files = [a for i, a in enumerate(args) if a != "--match" and (i == 0 or args[i - 1] != "--match")]
    tabs = [kernels(f) for f in files]
    names = list(tabs[-1])
    for n in tabs[0]:
        if n not in tabs[-1]:
            names.append(n)
    pretty = demangle(names)
    col = lambda k: f"{k['all']:6d} / {k['valu']:5d} / {k['scalar']:5d} / {k['lanes']:3d}  {k['vgpr']:4d} / {k['scratch']:3d}"  # noqa: E731
    worse = []
    for n in names:
        if not pat.search(pretty[n]):
            continue
        cells = [(col(t[n]) if n in t else f"{'(new)' if t is tabs[0] else '(gone)':>41}") for t in tabs]
        print(f"  {pretty[n]:<58}" + "    ".join(cells))
        if len(tabs) == 2 and n in tabs[0] and n in tabs[1]:
            if tabs[1][n]["vgpr"] > tabs[0][n]["vgpr"] or tabs[1][n]["scratch"] > tabs[0][n]["scratch"]:
                worse.append(pretty[n])
    if len(tabs) == 2:
        print("  more VGPRs or scratch on the right: " + (", ".join(worse) if worse else "none"))


if __name__ == "__main__":
    main()
