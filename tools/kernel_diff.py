"""Compare the gfx950 device code of two builds of the library: per code object the .text bytes, the kernel names with
VGPR / SGPR / LDS / scratch (the notes), and every kernel's own bytes (sliced from .text by its symbol).  Prints the
counts and, for every kernel that differs, how many instructions differ and the first differing pair.  It only
compares: what a difference means is for the reader.

    python tools/kernel_diff.py a/libboxattn_hip.so b/libboxattn_hip.so"""
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_objects


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def load(co):
    """-> (.text bytes, {kernel: (vgpr, sgpr, lds, scratch)}, {kernel: its bytes}, {kernel: [instruction, ...]})"""
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".text=" + co + ".text", co, "-"], check=True,
                   stdout=subprocess.DEVNULL)
    text = open(co + ".text", "rb").read()
    res = {}
    for k in re.split(r"\n\s+- \.agpr_count", run(LLVM + "/llvm-readelf", "--notes", co))[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, k).group(1)
        res[g("name")] = (g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"))
    base = int(re.search(r"\s\.text\s+PROGBITS\s+([0-9a-f]+)", run(LLVM + "/llvm-readelf", "-SW", co)).group(1), 16)
    code = {}
    for ln in run(LLVM + "/llvm-readelf", "-sW", co).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in res:
            a = int(f[1], 16) - base
            code[f[7]] = text[a:a + int(f[2], 0)]
    insts, cur = {}, None
    for ln in run(LLVM + "/llvm-objdump", "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = insts.setdefault(m.group(1), [])
        elif cur is not None and "//" in ln:
            cur.append(" ".join(ln.split("//")[0].split()))
    return text, res, code, insts


def main():
    a_path, b_path = sys.argv[1:3]
    ta, tb = tempfile.mkdtemp(), tempfile.mkdtemp()
    cos_a, cos_b = code_objects(a_path, ta), code_objects(b_path, tb)
    print("code objects: %d / %d" % (len(cos_a), len(cos_b)))
    n_kernels = n_differ = n_res = n_only = 0
    for i, (ca, cb) in enumerate(zip(cos_a, cos_b)):
        text_a, res_a, code_a, ins_a = load(ca)
        text_b, res_b, code_b, ins_b = load(cb)
        same_names = sorted(res_a) == sorted(res_b)
        print("code object %d: .text %d / %d bytes, %s; kernels %d / %d, names %s" % (
            i, len(text_a), len(text_b), "identical" if text_a == text_b else "DIFFERENT", len(res_a), len(res_b),
            "identical" if same_names else "DIFFERENT"))
        for name in sorted(set(res_a) ^ set(res_b)):
            n_only += 1
            print("  only in %s: %s" % ("A" if name in res_a else "B", name))
        for name in sorted(set(res_a) & set(res_b)):
            n_kernels += 1
            if res_a[name] != res_b[name]:
                n_res += 1
                print("  resources (vgpr, sgpr, lds, scratch) %s -> %s: %s" % (res_a[name], res_b[name], name))
            if code_a[name] == code_b[name]:
                continue
            n_differ += 1
            ia, ib = ins_a[name], ins_b[name]
            pairs = [(x, y) for x, y in zip(ia, ib) if x != y]
            print("  differs: %s" % name)
            print("    instructions %d / %d, mnemonic sequence %s, %d differ, mnemonics of those: %s" % (
                len(ia), len(ib), "identical" if [x.split()[0] for x in ia] == [y.split()[0] for y in ib] else "DIFFERENT",
                len(pairs), " ".join(sorted({x.split()[0] for x, _ in pairs}))))
            if pairs:
                print("    first: %s\n       ->  %s" % pairs[0])
    print("%d kernels in both, %d with different resources, %d of %d kernels differ" % (n_kernels, n_res, n_differ, n_kernels))
    return 1 if (n_differ or n_res or n_only or len(cos_a) != len(cos_b)) else 0


if __name__ == "__main__":
    sys.exit(main())
