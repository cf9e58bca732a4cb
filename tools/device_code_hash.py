"""sha256 of the gfx950 device code of every translation unit, product and -DFDN_TEST_HOOKS flavour: what a host-only refactor must
leave unchanged.  No GPU needed.   python tools/device_code_hash.py [--jobs N] [unit.hip ...]

Each unit is compiled device-only (build.FLAGS + --offload-device-only --no-gpu-bundle-output -c: a plain gfx950 ELF) and its .text
and .rodata sections are hashed.  One line per unit and flavour: `<unit> <product|test> text=<sha256> rodata=<sha256>` ("-": no such
section).  Run it on both trees and diff the output."""
import hashlib
import importlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
build = importlib.import_module("4dflownet_amd.build")


def _objcopy():
    hipcc = build._hipcc()
    real = os.path.realpath(hipcc) if os.path.isabs(hipcc) else hipcc
    for d in (os.path.join(os.path.dirname(os.path.dirname(real)), "lib", "llvm", "bin"), "/opt/rocm/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, "llvm-objcopy")):
            return os.path.join(d, "llvm-objcopy")
    return "llvm-objcopy"


def _section_hash(objcopy, elf, section, tmp):
    out = os.path.join(tmp, os.path.basename(elf) + section.replace(".", "_"))
    subprocess.run([objcopy, "-O", "binary", "--only-section=" + section, elf, out], check=True, capture_output=True)
    data = open(out, "rb").read() if os.path.exists(out) else b""
    return hashlib.sha256(data).hexdigest() if data else "-"


def unit_hashes(src, test_hooks, objcopy, tmp):
    elf = os.path.join(tmp, "%s.%s.elf" % (src, "test" if test_hooks else "product"))
    cmd = [build._hipcc(), "-x", "hip", "-c", os.path.join(build.CSRC, src), "-o", elf] + build.FLAGS + \
          ["--offload-device-only", "--no-gpu-bundle-output"] + (["-DFDN_TEST_HOOKS"] if test_hooks else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, r.stdout, r.stderr))
    return _section_hash(objcopy, elf, ".text", tmp), _section_hash(objcopy, elf, ".rodata", tmp)


def main(argv):
    jobs, units = 4, []
    it = iter(argv)
    for a in it:
        if a == "--jobs":
            jobs = int(next(it))
        else:
            units.append(a)
    units = units or build.SOURCES
    objcopy = _objcopy()
    cases = [(u, t) for u in units for t in (False, True)]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=jobs) as ex:
        for (u, t), (text, rodata) in zip(cases, ex.map(lambda c: unit_hashes(c[0], c[1], objcopy, tmp), cases)):
            print("%s %s text=%s rodata=%s" % (u, "test" if t else "product", text, rodata), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
