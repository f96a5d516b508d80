#!/usr/bin/env python3
"""Compare the compiled kernels of two builds, listing against listing: for a refactor that moves
kernels between translation units and must not change their code.

  tools/compare_kernel_listings.py <before_dir> <after_dir> [--may-differ REGEX]

Each directory holds one device listing per translation unit (<unit>.s, written by
`hipcc --offload-arch=gfx950 <flags> --cuda-device-only -S`, or <unit>-hip-amdgcn-*.s from `make asm`).
Units present on both sides are compared byte for byte first.  Then every kernel (.amdhsa_kernel
symbol) of <before_dir> is looked up in whichever unit of <after_dir> holds it and its function body,
from its label to .Lfunc_end, is compared with what counts functions or labels over the whole unit
normalised: the function index of the local labels (.LBB<k>_<j>, .Lfunc_end<k>, also where comments
name them) and the number of .Lpost_getpc<i>.  A kernel that differs is printed with its register
count, scratch and code size on both sides.  Exit status 1 if a kernel is missing or differs and
its symbol does not match --may-differ."""
import argparse
import re
import sys
from pathlib import Path

COUNTED = re.compile(r"(BB|\.Lfunc_end|\.Lpost_getpc|\.LJTI|\.LCPI)\d+")


def kernels(path: Path):
    """{symbol: (body lines, resource figures)} of one listing."""
    lines = path.read_text().split("\n")
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), flags=re.M))
    out, i = {}, 0
    while i < len(lines):
        sym = lines[i][:-1] if lines[i].endswith(":") else lines[i].split(":")[0]
        if sym in names and lines[i].startswith(sym + ":") and sym not in out:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            # (... and the padding in front of a comment, which follows the label's width)
            body = [re.sub(r"\s+;", " ;", COUNTED.sub(r"\1#", l)) for l in lines[i:end + 1]]
            fig = {}
            for l in lines[end:end + 60]:
                m = re.match(r"; (NumVgprs|NumAgprs|ScratchSize|codeLenInByte)\s*[:=]\s*(\d+)", l)
                if m:
                    fig.setdefault(m.group(1), int(m.group(2)))
            out[sym] = (body, fig)
            i = end
        i += 1
    assert set(out) == names, (path.name, sorted(names - set(out))[:3])
    return out


def unit(path: Path) -> str:
    return re.sub(r"-hip-amdgcn.*", "", path.stem)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("before", type=Path)
    ap.add_argument("after", type=Path)
    ap.add_argument("--may-differ", default=None, help="kernels (regex on the symbol) allowed to differ")
    a = ap.parse_args()
    before = {unit(p): p for p in sorted(a.before.glob("*.s"))}
    after = {unit(p): p for p in sorted(a.after.glob("*.s"))}
    same_units = [u for u in before if u in after and before[u].read_bytes() == after[u].read_bytes()]
    print("units byte-identical:", " ".join(same_units) or "-")
    print("units changed, added or removed:", " ".join(sorted((set(before) ^ set(after)) |
          {u for u in before if u in after and u not in same_units})) or "-")
    new = {}
    for u, p in after.items():
        for sym, k in kernels(p).items():
            new.setdefault(sym, (u, *k))
    old_syms = set()
    identical = moved = 0
    bad = []
    for u, p in before.items():
        if u in same_units:
            old_syms.update(kernels(p))
            continue
        for sym, (body, fig) in kernels(p).items():
            old_syms.add(sym)
            if sym not in new:
                print(f"MISSING  {sym} ({u})")
                bad.append(sym)
                continue
            nu, nbody, nfig = new[sym]
            if nbody == body:
                identical += 1
                moved += nu != u
                continue
            allowed = a.may_differ and re.search(a.may_differ, sym)
            print(f"{'differs (allowed)' if allowed else 'DIFFERS'}  {sym}\n    {u}: {fig}\n    {nu}: {nfig}")
            if not allowed:
                bad.append(sym)
    added = sorted(set(new) - old_syms)
    print(f"kernels of the changed units: {identical} identical ({moved} of them in another unit), "
          f"{len(bad)} missing or different, {len(added)} new")
    for sym in added:
        print("NEW     ", sym, f"({new[sym][0]})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
