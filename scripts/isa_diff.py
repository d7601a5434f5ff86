"""Is a change of the kernel sources a change of the device code?  (no GPU needed)
Usage: python scripts/isa_diff.py <tree A> <tree B> [--renames FILE] [file.hip ...]        (default: cg.hip cg_slab.hip)
Compiles each file of both trees (<tree>/differentiable-piso_amd/csrc) to gfx950 assembly with the library's flags, masks what
differs between any two compilations (comments, .file / .ident / .loc, the __hip_cuid_<hash> symbol, the numbers of .LBB / .Lfunc
labels) and prints a class per kernel:
  A  the masked text is identical
  B  the opcode histogram and the resource notes (VGPRs, SGPRs, both spill counts, scratch, LDS, kernarg size) are identical:
     the same instructions in another order
  C  anything else, with the counts that differ
Exit status: 0 if no kernel is of class C, 1 if one is, 2 if the two trees do not define the same kernels (the kernels of both are
still classified, and the resource notes of those only tree B has are listed).
--renames FILE: lines of `old symbol new symbol` (mangled names).  A kernel tree A calls `old` and tree B calls `new` is compared with its
predecessor under the old name (the new name in its text reads as the old one, section directives left out), not reported as
"only in A / only in B"; a class C kernel's instruction count is printed too."""
import collections, os, re, subprocess, sys, tempfile

from isa_loop import mix

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]     # = build_native.py
NOTES = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size",
         ".group_segment_fixed_size", ".kernarg_segment_size")


def start(tree, src, out):
    path = os.path.join(tree, "differentiable-piso_amd", "csrc", src)
    return subprocess.Popen(["/opt/rocm/bin/hipcc"] + FLAGS + ["-S", "--cuda-device-only", path, "-o", out], stderr=subprocess.PIPE,
                            universal_newlines=True)


def masked(text):
    out = []
    for l in text.split("\n"):
        l = l.split(";")[0].rstrip()                       # comments (no string of the device code holds a ';')
        if not l or re.match(r"\s*\.(file|ident|loc)\b", l):
            continue
        l = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", l)
        out.append(re.sub(r"\.L(BB|func_begin|func_end)\d+(_\d+)?", r".L\1", l))
    return out


def kernels(text):
    """{kernel symbol: (masked lines of its body, its resource notes)}"""
    notes = {}
    for entry in text.split(".amdgpu_metadata")[1].split("  - .agpr_count:")[1:]:
        name = re.search(r"\.symbol:\s+(\S+)\.kd", entry).group(1)
        notes[name] = {k: int(re.search(r"\s%s:\s+(\d+)" % re.escape(k), entry).group(1)) for k in NOTES}
    out = {}
    for name in notes:
        i = text.index("\n" + name + ":")
        out[name] = (masked(text[i:text.index(".Lfunc_end", i)]), notes[name])
    return out


def main():
    a, b = sys.argv[1], sys.argv[2]
    rest = sys.argv[3:]
    renames = []
    if rest and rest[0] == "--renames":
        renames = [l.split() for l in open(rest[1]) if l.strip()]
        rest = rest[2:]
    files = rest or ["cg.hip", "cg_slab.hip"]
    d = tempfile.mkdtemp(prefix="isa_diff_")
    jobs = [(f, t, os.path.join(d, "%s.%d.s" % (f, n)), None) for f in files for n, t in enumerate((a, b))]
    jobs = [(f, t, o, start(t, f, o)) for f, t, o, _ in jobs]
    for f, t, o, p in jobs:
        err = p.communicate()[1]
        if p.returncode != 0:
            sys.stderr.write("%s of %s does not compile:\n%s" % (f, t, err[-4000:]))
            raise SystemExit(2)
    status = 0
    for f in files:
        ka, kb = (kernels(open(os.path.join(d, "%s.%d.s" % (f, n))).read()) for n in (0, 1))
        renamed = {}
        for old, new in renames:
            if old in ka and new in kb and old not in kb:
                lines, notes = kb.pop(new)                 # (a template's kernel lies in a section of its own: the directive is no code)
                section = re.compile(r"\s*\.(text|section)\b")
                kb[old] = ([l.replace(new, old) for l in lines if not section.match(l)], notes)
                ka[old] = ([l for l in ka[old][0] if not section.match(l)], ka[old][1])
                renamed[old] = new
        if sorted(ka) != sorted(kb):
            print("%s: the kernel symbols differ: only in A %s, only in B %s" % (f, sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))))
            status = 2
            for name in sorted(set(kb) - set(ka)):         # what a new kernel takes: the resource notes of its metadata
                print("new  %s  %s  %s" % (f, name, ", ".join("%s %d" % (k[1:], kb[name][1][k]) for k in NOTES)))
        count = collections.Counter()
        for name in sorted(set(ka) & set(kb)):             # (kernels of one tree only were listed above: the rest is still compared)
            (la, na), (lb, nb) = ka[name], kb[name]
            ha, hb = mix(la), mix(lb)
            cls = "A" if la == lb else ("B" if ha == hb and na == nb else "C")
            count[cls] += 1
            if cls == "A" and not os.environ.get("ISA_DIFF_ALL"):
                continue
            print("%s  %s  %s%s" % (cls, f, name, "  ->  " + renamed[name] if name in renamed else ""))
            if cls == "C":
                status = max(status, 1)
                print("     notes: " + (", ".join("%s %d -> %d" % (k[1:], na[k], nb[k]) for k in NOTES if na[k] != nb[k]) or "equal"))
                print("     opcodes: " + (", ".join("%s %d -> %d" % (k, ha[k], hb[k]) for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]) or "equal"))
                if renames:
                    print("     instructions %d -> %d, vgpr %d -> %d, sgpr %d -> %d" % (sum(ha.values()), sum(hb.values()), na[".vgpr_count"], nb[".vgpr_count"],
                                                                                     na[".sgpr_count"], nb[".sgpr_count"]))
        print("%s: %d kernels (%d cg_persist1), class A %d, B %d, C %d%s" % (f, len(set(ka) & set(kb)), sum("cg_persist1" in k for k in ka), count["A"], count["B"], count["C"],
                                                                          ", %d of them renamed" % len(renamed) if renames else ""))
    raise SystemExit(status)


if __name__ == "__main__":
    main()
