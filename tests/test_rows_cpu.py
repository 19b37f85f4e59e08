"""csrc/rows.h on the host, no GPU: tools/rows_host_check.cpp (the rows description's refusals, statuses and messages,
the column packing) built as a stand-alone program with AddressSanitizer and UBSan by the compiler the library is built
with (ROCm's clang++ under ROCM_PATH, default /opt/rocm: where it is missing the library cannot be built either, and
this test fails rather than skips), and run."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_rows_host_check_under_sanitizers(tmp_path):
    exe = tmp_path / "rows_host_check"
    subprocess.run([os.path.join(ROCM, "llvm", "bin", "clang++"), "-std=c++17", "-g", "-O1",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(REPO, "retrieval-based-voice-conversion-mlx_amd", "csrc"),
                    os.path.join(REPO, "tools", "rows_host_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "rows.h host checks passed" in r.stdout, r.stdout + r.stderr
