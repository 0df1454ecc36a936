"""pw_xxh64_tagged2 (xxhash_common.h) on the host: tests/native/
xxh_tagged_check.cpp compares it with pw_xxh64_bytes over tag || bytes for
every len 0..130, start offset 0..7 and base misalignment 0..3, on heap
blocks of exactly the buffer's size.  The program is built with
AddressSanitizer and UBSan and run as a child process, so a load outside
the buffer ends it with an error."""

from __future__ import annotations

import os
import shutil
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "native", "xxh_tagged_check.cpp")
_INC = os.path.join(os.path.dirname(_HERE), "pathway_amd", "ops", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_tagged_hash_matches_bytes_hash_under_sanitizers(tmp_path):
    exe = str(tmp_path / "xxh_tagged_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         # the sanitizer runtimes are linked into the program, so nothing
         # in the environment has to be ordered around them
         "-static-libasan", "-static-libubsan",
         "-I", _INC, _SRC, "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 131 lengths x 8 offsets x 4 misalignments x 3 placements, and the
    # direct checks of the boundary dwords (3 misalignments x 8 lengths x 2)
    assert r.stdout.strip() == f"ok {131 * 8 * 4 * 3 + 3 * 8 * 2}", r.stdout + r.stderr
