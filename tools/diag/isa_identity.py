#!/usr/bin/env python3
"""Do two source trees compile to the same code?   tools/diag/isa_identity.py OLD_TREE NEW_TREE [--jobs N] [--keep DIR]

For each tree the compile commands come from `make -n -B all kmprof` in staticfusion_amd/csrc (so the Makefile is part of
what is compared). Every `hipcc ... -c -o X.o` command is run again with `--cuda-device-only -S`, and for the objects that
are not frame objects (the host side of the library) with `--cuda-host-only -S` as well. The hash of a compilation -- in
`__hip_cuid_<hash>` on the device side, `__hip_fatbin_<hash>` and `__hip_gpubin_handle_<hash>` on the host side: all that differs
between two compilations of the same source -- is replaced by a fixed token, and the assembly is compared object by object.
Required: the same object names in both trees and no difference at all.

Should a change of include order permute whole functions, the objects are compared once more function by function with
the `.LBB<n>_` label numbers normalised, and the report says `identical per function`. Anything else is `DIFFERENT` and
the exit status is 1. Where the device side of an object is DIFFERENT because one tree has functions the other lacks (a kernel
that moved to another object), one more line says whether every function both trees have is identical -- code, kernel
descriptor and metadata entry, with the `.Lfunc_end<n>` numbers normalised too -- and names the others. The exit status
stays 1: whether the move was intended is the reader's to judge. Needs hipcc, no GPU.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("staticfusion_amd", "csrc")
CUID = re.compile(r"__hip_(cuid|fatbin|gpubin_handle)_[0-9a-f]+")  # one hash per compilation: the device side's symbol, the host side's two
LBB = re.compile(r"\.LBB\d+_")
FUNC_BEGIN = re.compile(r"^([A-Za-z_$][\w$.]*):")


def compile_commands(tree):
    """object name -> argv of its compile command, as the tree's Makefile would run it"""
    out = subprocess.run(["make", "-n", "-B", "all", "kmprof"], cwd=os.path.join(tree, CSRC), check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or "-o" not in argv or "hipcc" not in os.path.basename(argv[0]):
            continue
        cmds[os.path.basename(argv[argv.index("-o") + 1])] = argv
    return cmds


def assemble(tree, argv, side, dst):
    argv = list(argv)
    argv[argv.index("-c")] = "-S"
    argv[argv.index("-o") + 1] = dst
    subprocess.run(argv + ["--cuda-%s-only" % side], cwd=os.path.join(tree, CSRC), check=True, capture_output=True, text=True)
    with open(dst) as f:
        return [CUID.sub(r"__hip_\1_X", l.rstrip("\n")) for l in f]


def instruction_lines(asm):
    n = 0
    for l in asm:
        t = l.strip()
        if l[:1] in " \t" and t and t[0] not in ".;#/" and not t.endswith(":"):
            n += 1
    return n


def by_function(asm):
    """symbol -> its lines with the block label numbers normalised; what lies outside any function under ''"""
    parts, cur = {"": []}, ""
    for l in asm:
        m = FUNC_BEGIN.match(l)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            parts.setdefault(cur, [])
        if l.startswith(".Lfunc_end"):
            parts[cur].append(LBB.sub(".LBB_", l))
            cur = ""
            continue
        parts[cur].append(LBB.sub(".LBB_", l))
    return parts


def common_functions(old, new):
    """for two device-side listings: (functions only old, only new, functions both have that differ)"""
    def parts(asm):
        out, kd, meta, in_meta = {}, None, None, False
        for name, lines in by_function(asm).items():
            if name and not name.startswith(("amdhsa.", "__hip_cuid")):
                out[name] = [re.sub(r"\.Lfunc_(begin|end)\d+|\bBB\d+_", "N_", l) for l in lines]  # (BB<n>_: in the loop comments)
        for l in asm:
            if l.strip().startswith(".amdhsa_kernel "):
                kd = out.setdefault(l.split()[1] + " (descriptor)", [])
            if kd is not None:
                kd.append(l)
            if l.strip() == ".end_amdhsa_kernel":
                kd = None
            if l.startswith("amdhsa.kernels:"):
                in_meta = True
            elif in_meta and l.startswith("  - "):
                meta = []
            elif in_meta and not l.startswith(" "):
                in_meta = False
            if in_meta and meta is not None:
                meta.append(l)
                if l.strip().startswith(".name:"):
                    out[l.split()[1] + " (metadata)"] = meta
        return out
    fo, fn = parts(old), parts(new)
    return sorted(set(fo) - set(fn)), sorted(set(fn) - set(fo)), sorted(k for k in fn if k in fo and fo[k] != fn[k])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--keep", help="keep the assembly files in this directory")
    ns = ap.parse_args()
    trees = [os.path.abspath(ns.old_tree), os.path.abspath(ns.new_tree)]
    cmds = [compile_commands(t) for t in trees]
    names = [sorted(c) for c in cmds]
    print("objects: old %d, new %d" % (len(names[0]), len(names[1])))
    bad = 0
    if names[0] != names[1]:
        print("DIFFERENT object sets: only old %s, only new %s" % (sorted(set(names[0]) - set(names[1])), sorted(set(names[1]) - set(names[0]))))
        bad = 1
    work = ns.keep or tempfile.mkdtemp(prefix="isa_identity_")
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(ns.jobs) as pool:
        for obj in sorted(set(names[0]) & set(names[1])):
            for side in ["device"] if obj.startswith("frame_") else ["device", "host"]:
                for k in range(2):
                    d = os.path.join(work, "old" if k == 0 else "new")
                    os.makedirs(d, exist_ok=True)
                    jobs[obj, side, k] = pool.submit(assemble, trees[k], cmds[k][obj], side, os.path.join(d, "%s.%s.s" % (obj[:-2], side)))
        print("%-28s %-7s %12s  %s" % ("object", "side", "instructions", "result"))
        for obj, side in sorted({(o, s) for o, s, _ in jobs}):
            try:
                old, new = jobs[obj, side, 0].result(), jobs[obj, side, 1].result()
            except subprocess.CalledProcessError as e:
                print("%-28s %-7s %12s  DID NOT COMPILE\n%s" % (obj, side, "-", e.stderr))
                bad = 1
                continue
            if old == new:
                verdict = "identical"
            elif sorted(by_function(old).items()) == sorted(by_function(new).items()):
                verdict = "identical per function (whole functions in another order; .LBB<n>_ numbers normalised)"
            else:
                verdict = "DIFFERENT"
                bad = 1
            print("%-28s %-7s %12d  %s" % (obj, side, instruction_lines(new), verdict))
            if verdict == "DIFFERENT":
                sys.stdout.writelines(l + "\n" for l in list(difflib.unified_diff(old, new, "old", "new", lineterm="", n=1))[:60])
                if side == "device":
                    gone, came, differ = common_functions(old, new)
                    if (gone or came) and not differ:
                        print("%-28s %-7s every function both trees have is identical (code, descriptor, metadata); only old: %s; only new: %s"
                              % (obj, side, gone or "none", came or "none"))
    print("RESULT: %s" % ("DIFFERENT" if bad else "all identical"))
    return bad


if __name__ == "__main__":
    sys.exit(main())
