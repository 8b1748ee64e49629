"""Do two builds of one translation unit run the same instructions?  Compares, function by function, the instruction streams of two gfx950 assembly files
(hipcc ... --cuda-device-only -S): labels and the template arguments inside lili:: symbol names are normalised, directives and comments dropped.  Every function of the
FIRST file must have a function of the same base name with the identical stream in the second; functions only the second file has are listed.  Exit status 1 otherwise.

    F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math --cuda-device-only -S"
    (cd <parent checkout>/lili_om_amd/csrc && hipcc $F lili_window.hip -o /tmp/win_parent.s)
    (cd lili_om_amd/csrc && hipcc $F lili_window.hip -o /tmp/win_this.s)
    python tools/asm_same.py /tmp/win_parent.s /tmp/win_this.s
"""
import re
import sys

SYM = re.compile(r"_ZN4lili\d+([a-z_0-9]+?)(?:I[A-Za-z0-9_]*?E)?E[A-Za-z0-9_]*")


def norm(text):
    return SYM.sub(r"lili::\1", re.sub(r"\.L\w+", "L", text))


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_ZN4lili\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        code = line.split(";")[0].rstrip()
        if code.strip() and not code.strip().startswith("."):
            cur.append(norm(code))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for name, body in a.items():
        same = [n for n, other in b.items() if norm(n) == norm(name) and other == body]
        print(f"{norm(name):32s} {len(body):5d} instructions  " + (f"same in {len(same)} instantiation(s)" if same else "DIFFERENT"))
        bad += 0 if same else 1
    known = {norm(n) for n in a}
    print("only in the second file:", sorted({norm(n) for n in b} - known))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
