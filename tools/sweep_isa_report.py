#!/usr/bin/env python
"""What the compiler made of the LDS sweeps' loads: a report to read, not a test. Needs hipcc only, no GPU.

Compiles kinetica_jl_amd/csrc/kernels.hip for gfx950 (device code only, to assembly) and prints, for every
sweep_reg_kernel / sweep_gen_kernel instantiation, its VGPRs, scratch bytes and occupancy, then the order of the events
that decide how many bytes a wave keeps in flight: global loads, `s_waitcnt vmcnt(n)`, barriers, scratch traffic and the
first LDS atomic after any of them, basic block by basic block with the compiler's loop annotations. Loads return in
order, so a vmcnt wait that sits between two loads of one batch (no LDS atomic, no barrier in between) ends the batch
there: everything requested so far is waited for before the next load goes out. Such waits are marked and counted.
(Expected ones: sweep_gen_kernel's gather kb[index] needs the index pairs of its first load group, and the launch
prologue reads one value-dependent index per lane, once.)

  python tools/sweep_isa_report.py                    # every instantiation, summary + event lists
  python tools/sweep_isa_report.py --only '<8, 4, false, 1024>'
  python tools/sweep_isa_report.py --src other/tree/kinetica_jl_amd/csrc/kernels.hip -D KIN_SWEEP_ILP=5
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_to_asm(src, defines, hipcc):
    tmp = tempfile.mkdtemp(prefix="sweep_isa_")
    try:
        out = os.path.join(tmp, "kernels.s")
        cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
               "-Rpass-analysis=kernel-resource-usage", "-I", os.path.dirname(src)] + [f"-D{d}" for d in defines] + [src, "-o", out]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(p.stderr[-4000:])
        return open(out).read(), p.stderr
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def demangle(names, hipcc):
    filt = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-cxxfilt")
    filt = filt if os.path.exists(filt) else shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.split("\n")
    return {n: re.sub(r"^void kin::|\(.*$", "", d) for n, d in zip(names, out)}


def resources(remarks):
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split()[0]] = m.group(2)
    return res


def events(body):
    """[(kind, text)] of one kernel: kind in block / load / wait / barrier / scratch / atomic"""
    ev = []
    for line in body:
        s = line.strip()
        if re.match(r"\.LBB\d+_\d+:", s):
            note = s.split(";", 1)[1].strip() if ";" in s else ""
            ev.append(("block", s.split(":")[0] + ("   ; " + note if note else "")))
        elif s.startswith("global_load") or s.startswith("buffer_load"):
            ev.append(("load", s.split()[0]))
        elif s.startswith("s_waitcnt") and "vmcnt" in s:
            ev.append(("wait", re.sub(r"\s+", " ", s.split(";")[0]).strip()))
        elif s.startswith("s_barrier"):
            ev.append(("barrier", "s_barrier"))
        elif s.startswith("scratch_"):
            ev.append(("scratch", s.split()[0]))
        elif s.startswith("ds_add") and (not ev or ev[-1][0] != "atomic"):
            ev.append(("atomic", s.split()[0] + "   (first of a run of LDS atomics)"))
    return ev


def mark_mid_batch_waits(ev):
    """indices of vmcnt waits that have a load before them and a load behind them with no LDS atomic or barrier between"""
    bad = set()
    for i, (k, _) in enumerate(ev):
        if k != "wait":
            continue
        before = False
        for kk, _ in reversed(ev[:i]):
            if kk in ("atomic", "barrier"):
                break
            if kk == "load":
                before = True
                break
        after = False
        for kk, _ in ev[i + 1:]:
            if kk in ("atomic", "barrier"):
                break
            if kk == "load":
                after = True
                break
        if before and after:
            bad.add(i)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=os.path.join(ROOT, "kinetica_jl_amd", "csrc", "kernels.hip"))
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME[=VALUE]")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--only", default=None, help="substring of the demangled name, e.g. '<8, 4, false, 1024>'")
    ap.add_argument("--summary", action="store_true", help="resource table only")
    args = ap.parse_args()

    asm, remarks = compile_to_asm(args.src, args.defines, args.hipcc)
    res = resources(remarks)
    lines = asm.splitlines()
    starts = [(i, m.group(1)) for i, line in enumerate(lines)
              for m in [re.match(r"(_ZN3kin16sweep_(?:reg|gen)_kernel\w+):", line)] if m]
    names = demangle([n for _, n in starts], args.hipcc)
    kernels = []
    for i, n in starts:
        end = next(j for j in range(i, len(lines)) if lines[j].strip().startswith("s_endpgm"))
        ev = events(lines[i + 1:end])
        kernels.append((names[n], res.get(n, {}), ev, mark_mid_batch_waits(ev)))

    print(f"{'kernel':<50} {'VGPRs':>5} {'scratch':>7} {'waves/SIMD':>10} {'vmcnt waits inside a batch of loads':>36}")
    for name, r, ev, bad in kernels:
        print(f"{name:<50} {r.get('VGPRs', '?'):>5} {r.get('ScratchSize', '?'):>7} {r.get('Occupancy', '?'):>10} {len(bad):>36}")
    if args.summary:
        return
    for name, r, ev, bad in kernels:
        if args.only and args.only not in name:
            continue
        print(f"\n==== {name}: {r.get('VGPRs', '?')} VGPRs, {r.get('ScratchSize', '?')} bytes of scratch per lane, "
              f"{r.get('Occupancy', '?')} waves per SIMD")
        for i, (k, t) in enumerate(ev):
            if k == "block":
                print(t)
            else:
                print("    " + t + ("      <-- between two loads of one batch" if i in bad else ""))


if __name__ == "__main__":
    main()
