"""Compare the device code of two trees of this repository, kernel by kernel.  No GPU needed.

    python tools/device_code_diff.py PARENT_TREE RESULT_TREE [--only pile_runs_kernel.hip ...] [--jobs N]
                                     [--json FILE] [--show SUBSTRING ...]

For both trees every rala_amd/csrc/*.hip that holds a __global__ is compiled with the build's flags (rala_amd/build.py) plus
--cuda-device-only -S.  Each kernel's text is cut from its label to its .Lfunc_end, its own and every other mangled symbol and
the numbers of local labels (they count the functions of the file) are replaced by placeholders, comments are dropped, and the
result is hashed.
Per file: how many bodies both trees have, the kernels whose body only the parent / only the result has, and for every kernel
.vgpr_count, .sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size where a kernel of the same body differs
in them.  --show prints, for the kernels whose demangled name contains SUBSTRING and whose body differs (paired by that name),
the resources, the instruction counts by mnemonic that differ and the line diff of the normalised bodies.  --json writes name,
hash and resources of every kernel of both trees (a trace of kernel names can then be keyed by body).  The tool compares text; it searches for nothing.  Exit status 0 whatever it finds: the reader judges."""
import argparse
import collections
import difflib
import hashlib
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

RESOURCES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def hipcc():
    import shutil
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise SystemExit("hipcc not found")


def kernel_files(tree, only):
    d = os.path.join(tree, "rala_amd", "csrc")
    out = []
    for f in sorted(os.listdir(d)):
        if f.endswith(".hip") and (not only or f in only):
            with open(os.path.join(d, f)) as fh:
                if "__global__" in fh.read():
                    out.append(f)
    return out


def assemble(tree, f, tmp):
    d = os.path.join(tree, "rala_amd", "csrc")
    out = os.path.join(tmp, f[:-4] + ".s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(tree, "include"), "-I" + d]
    flags += shlex.split(os.environ.get("RALA_HIPCC_FLAGS", ""))
    res = subprocess.run([hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(d, f), "-o", out], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise SystemExit("compile failed: %s\n%s" % (f, res.stdout))
    with open(out) as fh:
        return fh.read()


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
        out = res.stdout.split("\n")
        if res.returncode == 0 and len(out) >= len(names):
            return dict(zip(names, out))
    except OSError:
        pass
    return {n: n for n in names}


def kernels_of(text):
    """-> {name: {"hash", "body" (normalised lines), resources ...}}"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    meta = {}
    for block in re.split(r"^  - \.", text[text.find(".amdgpu_metadata"):], flags=re.M)[1:]:
        m = re.search(r"^\s*\.name:\s*(\S+)", block, re.M)
        if m:
            meta[m.group(1)] = {k: int(re.search(r"%s:\s*(\d+)" % re.escape(k), "." + block).group(1)) for k in RESOURCES}
    out = {}
    for name in names:
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        body = m.group(0).replace(name, "SELF")
        body = re.sub(r"\b_Z\w+", "SYM", body)
        body = re.sub(r"\.L(BB|JTI|func_end|func_begin|tmp)\d+", r".L\1N", body)
        lines = [l for l in (re.sub(r"\s*;.*", "", l).rstrip() for l in body.split("\n")) if l]     # (comments name block numbers)
        out[name] = dict(meta.get(name, {}), hash=hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], body=lines)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("result")
    ap.add_argument("--only", nargs="*", default=[])
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--json")
    ap.add_argument("--show", nargs="*", default=[])
    a = ap.parse_args()
    trees = {"parent": os.path.abspath(a.parent), "result": os.path.abspath(a.result)}
    files = {t: kernel_files(p, a.only) for t, p in trees.items()}
    code = {}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=a.jobs) as pool:
        jobs = {}
        for t, p in trees.items():
            os.makedirs(os.path.join(tmp, t))
            for f in files[t]:
                jobs[t, f] = pool.submit(assemble, p, f, os.path.join(tmp, t))
        for key, job in jobs.items():
            code[key] = kernels_of(job.result())
    dem = demangle(sorted({n for k in code.values() for n in k}))
    dump = {t: {} for t in trees}
    total = [0, 0, 0]
    for f in sorted(set(files["parent"]) | set(files["result"])):
        P, R = code.get(("parent", f), {}), code.get(("result", f), {})
        for t, K in (("parent", P), ("result", R)):
            dump[t][f] = [dict({k: v for k, v in K[n].items() if k != "body"}, name=n, demangled=dem[n]) for n in sorted(K)]
        hp, hr = {}, {}
        for n, k in P.items():
            hp.setdefault(k["hash"], []).append(n)
        for n, k in R.items():
            hr.setdefault(k["hash"], []).append(n)
        common = [h for h in hp if h in hr]
        n_common = sum(min(len(hp[h]), len(hr[h])) for h in common)
        only_p = [n for h in hp for n in hp[h][len(hr.get(h, [])):]]
        only_r = [n for h in hr for n in hr[h][len(hp.get(h, [])):]]
        total = [total[0] + n_common, total[1] + len(only_p), total[2] + len(only_r)]
        print("%-28s parent %3d  result %3d  common %3d  only parent %2d  only result %2d" % (f, len(P), len(R), n_common, len(only_p), len(only_r)))
        for tag, K, lst in (("only in parent", P, only_p), ("only in result", R, only_r)):
            for n in sorted(lst, key=lambda n: dem[n]):
                print("    %s: %s\n        %s  %s" % (tag, dem[n], K[n]["hash"], " ".join("%s %s" % (k[1:], K[n].get(k)) for k in RESOURCES)))
        for h in common:
            rp, rr = ({tuple(K[n].get(k) for k in RESOURCES) for n in names} for K, names in ((P, hp[h]), (R, hr[h])))
            if rp != rr:
                print("    same body, other resources: %s parent %s result %s" % (dem[hp[h][0]], sorted(rp), sorted(rr)))
    print("all files: common %d, only parent %d, only result %d" % tuple(total))
    for s in a.show:
        for f in sorted(set(files["parent"]) & set(files["result"])):
            P, R = code["parent", f], code["result", f]
            short = lambda n: re.sub(r"\(.*", "", dem[n].replace("(anonymous namespace)", "{anonymous}"))      # (without the arguments)
            for n in sorted(P):
                if s not in dem[n]:
                    continue
                for m in sorted(R):
                    if short(m) == short(n) and P[n]["hash"] != R[m]["hash"]:
                        print("\n--- %s (parent) / %s (result), %s" % (dem[n], dem[m], f))
                        for k in RESOURCES:
                            print("    %-28s parent %6s  result %6s" % (k, P[n].get(k), R[m].get(k)))
                        # instructions by mnemonic (where a change moves registers about, the line diff is long and says little)
                        count = lambda body: collections.Counter(l.split()[0] for l in body if l.startswith("\t") and not l.startswith("\t."))
                        cp, cr = count(P[n]["body"]), count(R[m]["body"])
                        print("    instructions                 parent %6d  result %6d" % (sum(cp.values()), sum(cr.values())))
                        for op in sorted(set(cp) | set(cr)):
                            if cp[op] != cr[op]:
                                print("      %-26s parent %6d  result %6d  (%+d)" % (op, cp[op], cr[op], cr[op] - cp[op]))
                        sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(P[n]["body"], R[m]["body"], "parent", "result", lineterm="", n=2))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dump, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
