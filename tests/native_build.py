"""The list of libambrycrc's sources, as ambry_amd/Makefile derives it from csrc/, and the build of a
stand-alone harness program (tests/native/*.cpp) with the library's host code under ASan + UBSan."""
import glob
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ambry_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_ONLY = "host_crc.cpp"  # x86 CLMUL intrinsics: the host compiler's, never compiled as HIP


def library_sources():
    """Every csrc/*.cpp but the host compiler's one, then every csrc/*.hip (the Makefile's CPPSRC, HIPSRC)."""
    cpp = [p for p in sorted(glob.glob(os.path.join(CSRC, "*.cpp"))) if os.path.basename(p) != HOST_ONLY]
    return cpp + sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def have_toolchain():
    return os.path.exists(HIPCC) and shutil.which("g++") is not None


def build_sanitized(harness, exe, tmp_path):
    """Links `harness` (a file of tests/native/) and the whole library into the program `exe`: the host CRC
    loops by g++ and the library sources by hipcc, host side under AddressSanitizer + UBSan (-Xarch_host:
    the device code is compiled as always)."""
    host_o = os.path.join(str(tmp_path), "host_crc.o")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fPIC",
                    "-std=c++17", "-c", os.path.join(CSRC, HOST_ONLY), "-o", host_o], check=True, timeout=300)
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950",
                    "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", host_o,
                    os.path.join(ROOT, "tests", "native", harness)] + library_sources() + ["-ldl", "-o", str(exe)],
                   check=True, timeout=900)
