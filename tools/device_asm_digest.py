#!/usr/bin/env python3
"""Digest of the gfx950 device code of every log_amd/csrc/*.hip: `file  sha256`, one line per source.

    python tools/device_asm_digest.py [TREE]        (TREE: a checkout of this repository, default: this one)

Each source is compiled with the flags of log_amd/build.py plus `--cuda-device-only -S`, from TREE as the working
directory and under its relative path, so that two trees give comparable assembly.  Lines that contain `__hip_cuid_`
(a per-translation-unit symbol hashed from the whole file: the only thing a host-side edit moves) are dropped before
hashing.  A change that is meant to leave the kernels alone is checked by running this on the parent's tree and on the
changed one and comparing the two lists.
"""
import glob
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from log_amd.build import FLAGS, HIPCC  # noqa: E402


def digest(tree, src):
    asm = subprocess.check_output([HIPCC] + FLAGS + ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument", src, "-o", "-"], cwd=tree)
    kept = [ln for ln in asm.splitlines(keepends=True) if b"__hip_cuid_" not in ln]
    return hashlib.sha256(b"".join(kept)).hexdigest(), len(kept)


def main():
    tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
    srcs = sorted(os.path.relpath(p, tree) for p in glob.glob(os.path.join(tree, "log_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 4, 16)) as ex:
        for src, (sha, lines) in zip(srcs, ex.map(lambda s: digest(tree, s), srcs)):
            print(f"{src}  {sha}  ({lines} lines)")


if __name__ == "__main__":
    main()
