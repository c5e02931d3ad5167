"""What the host-build tests (tests/test_*_hostbuild.py) share: compiling a stand-alone program of tools/*_host_main.cpp with the library
build's own flags, plain or with the host's address and undefined-behaviour sanitizers, and running it as a child process. No sanitizer is
loaded into Python and no GPU is involved."""

import os
import subprocess

from gtsfm_amd.csrc.build import FLAGS as BUILD_FLAGS
from gtsfm_amd.csrc.build import HIPCC

FLAGS = [f for f in BUILD_FLAGS if f != "-fPIC"]  # an executable, not a shared library
SANITIZE = "-fsanitize=address,undefined"


def build_program(tmp_path_factory, source, sanitized):
    """(executable, its directory) of ``source``, e.g. tools/view_graph_host_main.cpp -> view_graph_host."""
    name = source.stem.removesuffix("_main")
    d = tmp_path_factory.mktemp(f"{name}_{'sanitized' if sanitized else 'plain'}")
    obj, exe = d / "main.o", d / name
    # the device side ignores the host-only flag; the link step takes it plain
    subprocess.run([HIPCC, *FLAGS, *(["-Xarch_host", SANITIZE] if sanitized else []), "-c", str(source), "-o", str(obj)], check=True, capture_output=True, timeout=600)
    subprocess.run([HIPCC, *([SANITIZE] if sanitized else []), str(obj), "-o", str(exe)], check=True, capture_output=True, timeout=600)
    return exe, d


def run(exe, args, expect_status=0):
    """The finished process: its exit status is ``expect_status`` and no sanitizer spoke."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    done = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600, env=env)
    assert done.returncode == expect_status, f"exit status {done.returncode}\n{done.stderr[-3000:]}"
    assert "runtime error" not in done.stderr and "Sanitizer" not in done.stderr, done.stderr[-3000:]
    return done
