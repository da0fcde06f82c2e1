"""Are the device code objects of two source trees the same?  For a change that must not touch a kernel.

    python tools/code_object_diff.py OTHER_TREE/swmhd_amd/csrc [swmhd_amd/csrc] [--json out.json]

For every translation unit of the Makefile's OBJS the device side alone is compiled in both directories with the command line `make -n`
prints for that unit (plus --offload-device-only --no-gpu-bundle-output), then `llvm-objdump -d --no-show-raw-insn` and `llvm-readelf --notes` of the two code
objects are compared.  Lines that carry the object's path or the __hip_cuid_* symbol (a hash of the path) are left out.  Needs no GPU.
Per unit also `opcodes_equal`: the sequence of instruction mnemonics, label and symbol lines included, operands ignored (a listing
that differs only in registers or in the order of a commutative operation's sources has it), and `differing_lines`, the count of
listing lines that differ, and `mix_equal`: symbol by symbol the same count of every mnemonic (instructions moved, none added).  A unit that only one of the two Makefiles builds is reported as {"only_in": "mine" | "other"} and not
compared: a change that adds a kernel leaves every older unit to be shown equal.
Exit status 0: all equal."""
import concurrent.futures
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
HERE = os.path.dirname(os.path.abspath(__file__))


def units(csrc):
    out = subprocess.run(["make", "-C", csrc, "-n", "-B", "../libswmhd.so"], capture_output=True, text=True, check=True).stdout
    cmds = {}
    for line in out.splitlines():
        m = re.search(r"-c (\S+)\.hip -o (\S+)\.o$", line)
        if m:
            cmds[m.group(2)] = line.split()      # by object: diffusion.hip and coriolis.hip are each built twice
    return cmds


def device_listing(csrc, unit, cmd, tmp):
    co = os.path.join(tmp, unit + ".co")
    cmd = [c for c in cmd[:-1]] + [co]
    cmd[1:1] = ["--offload-device-only", "--no-gpu-bundle-output"]
    subprocess.run(cmd, cwd=csrc, check=True, capture_output=True)
    text = []
    for tool in (["llvm-objdump", "-d", "--no-show-raw-insn"], ["llvm-readelf", "--notes"]):
        r = subprocess.run([os.path.join(ROCM_LLVM, tool[0])] + tool[1:] + [co], capture_output=True, text=True, check=True)
        text.append([l for l in r.stdout.splitlines() if co not in l and "file format" not in l and "__hip_cuid_" not in l])
    return text


def opcodes(listing):
    """The first word of every line of a disassembly: the mnemonic of an instruction, the whole of a label or symbol line"""
    return [l if l.rstrip().endswith(":") else l.split()[0] for l in listing if l.strip()]


def mix(listing):
    """Per symbol of a disassembly, how often each instruction mnemonic occurs in it: what a reordering of instructions leaves alone"""
    out, sym = {}, None
    for l in listing:
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", l.strip())
        if m:
            sym = out.setdefault(m.group(1), {})
        elif l.strip() and not l.rstrip().endswith(":") and sym is not None:
            sym[l.split()[0]] = sym.get(l.split()[0], 0) + 1
    return out


def differing_lines(a, b):
    if a == b:
        return 0
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def main(argv):
    js = None
    if "--json" in argv:
        k = argv.index("--json")
        js = argv[k + 1]
        del argv[k:k + 2]
    other = os.path.abspath(argv[0])
    mine = os.path.abspath(argv[1] if len(argv) > 1 else os.path.join(HERE, "..", "swmhd_amd", "csrc"))
    cmds = {d: units(d) for d in (other, mine)}
    both = sorted(set(cmds[other]) & set(cmds[mine]))
    report = {u: {"only_in": "mine" if u in cmds[mine] else "other"} for u in sorted(set(cmds[other]) ^ set(cmds[mine]))}
    for u, r in report.items():
        print(u, r, flush=True)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, concurrent.futures.ThreadPoolExecutor(8) as pool:
        jobs = {(d, u): pool.submit(device_listing, d, u, cmds[d][u], t) for d, t in ((other, ta), (mine, tb)) for u in both}
        for u in both:
            a, b = jobs[(other, u)].result(), jobs[(mine, u)].result()
            report[u] = {"disassembly_lines": len(b[0]), "notes_lines": len(b[1]), "disassembly_equal": a[0] == b[0], "notes_equal": a[1] == b[1],
                         "opcodes_equal": opcodes(a[0]) == opcodes(b[0]), "mix_equal": mix(a[0]) == mix(b[0]), "differing_lines": differing_lines(a[0], b[0])}
            print(u, report[u], flush=True)
    if js:
        with open(js, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")
    return 0 if all(r["disassembly_equal"] and r["notes_equal"] for r in report.values() if "only_in" not in r) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
