"""Developer tool: are the kernels two builds of libatcstep.so have in common the same machine code?

    python tools/isa_compare.py <a.so> <b.so> [regex of (mangled) kernel names, default: all shared symbols]

tools/codeobj_diff.sh compares whole code objects, which differ as soon as a kernel is added (addresses move).  This one splits the
gfx950 disassembly (llvm-objdump -d) by symbol and compares each shared symbol's ENCODED instruction words — branch offsets are
relative, so identical code at another address has identical words.  Alignment padding behind a symbol's last instruction (zero
words, s_nop, s_code_end) is dropped before comparing, so a difference in TRAILING s_nop alone is not seen; the summary line says so.
Prints one line per symbol that differs and a summary; exit status 1 if any differs."""
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")


def symbols(lib):
    with tempfile.TemporaryDirectory() as t:
        so = os.path.join(t, "x.so")
        with open(lib, "rb") as f, open(so, "wb") as g:
            g.write(f.read())
        subprocess.run([OBJDUMP, "--offloading", "x.so"], cwd=t, check=True, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(t) if "gfx950" in f]
        assert len(co) == 1, co
        text = subprocess.run([OBJDUMP, "-d", co[0]], cwd=t, check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and "//" in line:
            cur.append(line.split("//")[1].split(":", 1)[1].strip())   # the encoded words, without the address
    for words in out.values():   # alignment padding behind a symbol's last instruction (zero words, s_nop, s_code_end) is not code
        while words and words[-1].upper() in ("00000000", "BF800000", "BF9F0000"):
            words.pop()
    return out


def main():
    a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
    pat = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    shared = sorted(n for n in a if n in b and (pat is None or pat.search(n)))
    bad = [n for n in shared if a[n] != b[n]]
    for n in bad:
        print("DIFFERS %s (%d vs %d instructions)" % (n, len(a[n]), len(b[n])))
    for tag, x, y in (("ONLY IN A", a, b), ("ONLY IN B", b, a)):   # a kernel one build adds (k_adv_moments, k_adv_apply, k_adam_step over their parent)
        for n in sorted(n for n in x if n not in y and (pat is None or pat.search(n))):
            print("%s %s (%d instructions)" % (tag, n, len(x[n])))
    print("%d shared symbols compared (trailing padding / s_nop ignored), %d differ; only in a: %d, only in b: %d"
          % (len(shared), len(bad), len([n for n in a if n not in b]), len([n for n in b if n not in a])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
