"""DevBuf<T> (csrc/devbuf.h): the move-only owner of a hipMalloc allocation that every handle keeps its device tables in.  A stand-alone host program
(tests/cpp/devbuf_check.cpp, compiled by hipcc because the header includes the HIP runtime) holds it to its contract: a failed alloc / upload returns
-1, leaves the buffer empty and sets the error text; moves leave the source empty; reset() of an empty buffer and the destructor of a never-filled one
do nothing.  Without a device every hipMalloc fails, which is exactly the failure path; with one the program also round-trips a one-element and a
zero-element upload (non-null pointer, size 0).  It branches on its first hipMalloc, so it runs on either kind of machine.  The event and stream
owners of the same header (DevEvent, DevStream) are held to the same contract by the same program: without a device create() fails (-1, empty,
error text; moves and resets of empty owners are no-ops), with one an event is created, moved, recorded and waited for on the null stream, and a
stream is created with flags and priority and destroyed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_contract(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc")
    exe = os.path.join(str(tmp_path), "devbuf_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "devbuf_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    m = re.search(r"^OK device=([01]) checks=(\d+)$", r.stdout, flags=re.M)
    assert m and int(m.group(2)) >= 21, r.stdout


def test_the_header_is_host_code_on_the_runtime_alone():
    src = open(os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc", "devbuf.h")).read()
    assert set(re.findall(r'^#include\s+[<"]([^>"]+)[>"]', src, flags=re.M)) == {"hip/hip_runtime.h", "string", "vector"}
    assert "__global__" not in src and "__device__" not in src
