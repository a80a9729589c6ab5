"""Digest of the device code of every source of librs_asr.so, to prove that a host-only change left the kernels alone.

    python scripts/device_code_digest.py [--full]

Every file of build.SOURCES is compiled with the build's own flags plus --offload-device-only, the gfx950 code object is taken
out of the bundle, and a sha256 of its .text, .rodata and .note sections is printed (.note holds the kernels' register, LDS and
scratch metadata).  Run it on two commits and compare the tables: no GPU is needed.

The whole object file is useless for this: the compiler embeds an id derived from the source text, so a comment in a header
changes it.  The three sections do not change with it, nor with the directory the tree sits in.  The digests are cut to 16 hex
digits unless --full is given; the last line is one sha256 over the whole table.
"""
import concurrent.futures
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reazonspeech_amd import build  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")
TARGET = "hipv4-amdgcn-amd-amdhsa--" + build.ARCH


def _bundler():
    hipcc = build._hipcc()
    if os.path.sep in hipcc:
        cand = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang-offload-bundler")
        if os.path.exists(cand):
            return cand
    for cand in ("/opt/rocm/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        if os.path.exists(cand):
            return cand
    return "clang-offload-bundler"


def elf_sections(blob):
    """name -> bytes of every section of a little-endian ELF64 image that has contents in the file"""
    assert blob[:4] == b"\x7fELF" and blob[4] == 2 and blob[5] == 1, "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = blob[heads[shstrndx][4]:heads[shstrndx][4] + heads[shstrndx][5]]
    out = {}
    for name_off, kind, _flags, _addr, off, size, *_ in heads:
        if kind == 8:       # SHT_NOBITS
            continue
        out[names[name_off:names.index(b"\0", name_off)].decode()] = blob[off:off + size]
    return out


def digest(src, tmp):
    obj = os.path.join(tmp, src + ".o")
    elf = os.path.join(tmp, src + ".elf")
    cmd = [build._hipcc()] + build.COMMON + build.EXTRA.get(src, []) + ["--offload-device-only", "-c", os.path.join(build.CSRC, src), "-o", obj]
    subprocess.run(cmd, check=True, capture_output=True)
    subprocess.run([_bundler(), "--unbundle", "--type=o", "--input=" + obj, "--targets=" + TARGET, "--output=" + elf], check=True, capture_output=True)
    with open(elf, "rb") as f:
        sections = elf_sections(f.read())
    return [hashlib.sha256(sections[s]).hexdigest() if s in sections else "-" for s in SECTIONS]


def main():
    width = 64 if "--full" in sys.argv else 16
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        rows = list(ex.map(lambda s: digest(s, tmp), build.SOURCES))
    whole = hashlib.sha256()
    print(f"{'file':<22}" + "".join(f"{s:<{width + 2}}" for s in SECTIONS))
    for src, row in zip(build.SOURCES, rows):
        print(f"{src:<22}" + "".join(f"{h[:width]:<{width + 2}}" for h in row))
        whole.update((src + " " + " ".join(row) + "\n").encode())
    print("all " + whole.hexdigest())


if __name__ == "__main__":
    main()
