"""Build libsccsum.so in-tree with hipcc for gfx950.

SOURCES and headers() are the one list of what the library is made of: the
A/B builds (tools/build_ab.sh) and the sanitizer builds (tests/test_sanitize.py)
take them from here.
"""
from __future__ import annotations

import glob
import os
import subprocess

from .native import LIB_PATH, PKG_DIR, REPO_DIR

CSRC = os.path.join(PKG_DIR, "csrc")
SOURCES = [os.path.join(CSRC, f) for f in
           ("sccsum.hip", "steer.hip", "send.hip", "reasm.hip", "eth.hip", "udp.hip", "tcp.hip", "tcp_data.hip", "tcp_tx_data.hip", "tcp_ack.hip", "tcp_listen.hip", "checksummer.cc", "pipeline.cc", "burst.cc")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# The AMDGPU atomic optimizer rewrites the kernels' lane-0 atomics into
# wave-wide ones whose result it reads back where they are issued; the flat
# kernel's LATE form reads its tile claim back a tile later (sccsum.hip,
# flat_body).  No kernel has an atomic it would help: each is one lane's.
DEVICE_FLAGS = ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]


def headers() -> list[str]:
    """Every header the build reads: an edit to any of them makes the library stale."""
    return sorted(glob.glob(os.path.join(REPO_DIR, "include", "sccsum*.h")) + glob.glob(os.path.join(CSRC, "*.h")))


def hipcc_cmd(out: str = LIB_PATH) -> list[str]:
    return [
        HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared",
        "-Wall", "-Wno-unused-command-line-argument", *DEVICE_FLAGS,
        "-I", os.path.join(REPO_DIR, "include"),
        *SOURCES, "-o", out,
    ]


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    newest = max(os.path.getmtime(p) for p in SOURCES + headers())
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest:
        return LIB_PATH
    cmd = hipcc_cmd()
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB_PATH

