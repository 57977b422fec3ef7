#!/usr/bin/env python3
"""Developer tool (host only, no GPU): what hipcc made of the MFMA loops of the csrc kernels.

Compiles each given csrc file (default: conv3_halo.hip) for gfx950 with the Makefile's flags plus
`-S --cuda-device-only -Rpass-analysis=kernel-resource-usage` and prints, per kernel instance that has MFMAs:

  VGPRs / AGPRs / SGPRs / ScratchSize    from the resource-usage remarks
  scratch_load in loop                   scratch_load lines between the first and the last v_mfma of the instance
                                         ("spill": tagged Folded Reload / Reload by the register allocator, "other": a stack slot)
  entered with 0 reads in flight         MFMA runs that start with no LDS read outstanding, by a straight-line walk of the listing:
                                         every ds_read adds one, s_waitcnt lgkmcnt(N) caps the count at N
  histogram                              "R reads -> M MFMAs": R LDS reads issued since the previous MFMA run, M the length of the run
                                         that follows (a run = v_mfma lines with no ds_read between them).  "1 -> 4" many times over is
                                         the serialised form read, wait, 4 MFMAs; a pipelined loop shows the same pairs, but none of
                                         its runs is entered with 0 reads in flight except the last of a tap.

The walk follows the listing, not the control flow: loop bodies are counted once, and a run behind a branch target inherits the count
of the text above it.  The tap loops of conv3_halo / conv3_ws are fully unrolled per chunk, which is what the walk is meant for.

    python tools/halo_loop_isa.py [--filter SUBSTRING] [file.hip ...] > profiles/halo_loop_isa_after.txt

A full compile of conv3_halo.hip takes minutes."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-classifier_amd", "csrc")


def makefile_flags():
    """FLAGS of csrc/Makefile, $(ROOT) resolved."""
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"FLAGS\s*:=\s*(.*)", line)
        if m:
            return m.group(1).replace("$(ROOT)", ROOT).split()
    raise SystemExit("no FLAGS line in csrc/Makefile")


def demangle(names):
    """{mangled: readable}.  binutils' c++filt does not know the 16-bit float manglings, so they go in as vendor types."""
    import shutil
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    sub = [n.replace("DF16b", "u6__bf16").replace("DF16_", "u8_Float16") for n in names]
    try:
        out = subprocess.run([tool], input="\n".join(sub), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def resources(stderr):
    """{mangled name: {field: int}} from the kernel-resource-usage remarks."""
    res, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return res


def functions(asm):
    """(mangled name, [instruction lines]) for every function of the listing."""
    name, body = None, []
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name and line.startswith(".Lfunc_end"):
            yield name, body
            name = None
            continue
        if name is not None and line.startswith("\t") and not line.startswith("\t."):
            body.append(line.strip())


def walk(body):
    mf = [i for i, l in enumerate(body) if l.startswith("v_mfma")]
    if not mf:
        return None
    first, last = mf[0], mf[-1]
    spill = other = 0
    hist = collections.Counter()
    zero = runs = 0
    reads_since = outstanding = run = 0
    entered = 0
    for l in body[first:last + 1]:
        op = l.split()[0]
        if op.startswith("scratch_load"):
            if "Reload" in l:
                spill += 1
            else:
                other += 1
        if op.startswith("v_mfma"):
            if run == 0:
                entered = outstanding
            run += 1
            continue
        if op.startswith("ds_read") or op.startswith("ds_load"):
            if run:
                hist[(reads_since, run)] += 1
                runs += 1
                zero += entered == 0
                run = reads_since = 0
            reads_since += 1
            outstanding += 1
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", l)
            if m:
                outstanding = min(outstanding, int(m.group(1)))
    if run:
        hist[(reads_since, run)] += 1
        runs += 1
        zero += entered == 0
    return dict(mfma=len(mf), spill=spill, other=other, hist=hist, zero=zero, runs=runs)


def report(path, flt, defines=()):
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "out.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + makefile_flags() + [f"-D{d}" for d in defines] + [
            "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", path, "-o", s]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            sys.stderr.write(p.stderr)
            raise SystemExit(f"{os.path.basename(path)}: hipcc failed")
        asm = open(s).read()
    res = resources(p.stderr)
    funcs = [(n, b) for n, b in functions(asm) if n in res]
    names = demangle([n for n, _ in funcs])
    print(f"== {os.path.basename(path)}")
    rows = []
    for n, body in funcs:
        w = walk(body)
        if w is None or (flt and flt not in names[n]):
            continue
        rows.append((re.sub(r"^void |\(.*$", "", names[n]), res[n], w))
    for nm, r, w in sorted(rows, key=lambda t: t[0]):
        print(f"{nm}")
        print(f"    VGPRs {r.get('VGPRs', -1)}  AGPRs {r.get('AGPRs', -1)}  SGPRs {r.get('TotalSGPRs', -1)}  ScratchSize {r.get('ScratchSize', -1)} B/lane  "
              f"occupancy {r.get('Occupancy', -1)} waves/SIMD  MFMAs {w['mfma']}")
        print(f"    scratch_load between first and last MFMA: {w['spill'] + w['other']} (spill reloads {w['spill']}, other {w['other']})")
        print(f"    MFMA runs {w['runs']}, entered with 0 reads in flight: {w['zero']}")
        print("    reads -> MFMA run: " + "  ".join(f"{a}->{b} x{c}" for (a, b), c in sorted(w["hist"].items())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", default=["conv3_halo.hip"], help="csrc files (names inside csrc/ or paths)")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME[=VALUE]", help="extra preprocessor definitions (diagnostic builds)")
    a = ap.parse_args()
    for f in a.files:
        report(f if os.path.exists(f) else os.path.join(CSRC, f), a.filter, a.defines)


if __name__ == "__main__":
    main()
