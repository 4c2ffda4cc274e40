"""The list of libambrycrc's sources, as ambry_amd/Makefile derives it from csrc/, and the build of a
stand-alone harness program (tests/native/*.cpp) under ASan + UBSan: with the whole library (build_sanitized)
or with host-only sources named by the caller (build_host_sanitized). Every harness has its own main; nothing
here is loaded into Python."""
import glob
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ambry_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_ONLY = "host_crc.cpp"  # x86 CLMUL intrinsics: the host compiler's, never compiled as HIP
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# for a host-only harness that includes the library's headers: the HIP runtime's types, no device code
HIP_HEADERS = ("-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))


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
    subprocess.run(["g++"] + SANITIZE + ["-fPIC", "-std=c++17", "-c", os.path.join(CSRC, HOST_ONLY), "-o", host_o],
                   check=True, timeout=300)
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950",
                    "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", host_o,
                    os.path.join(ROOT, "tests", "native", harness)] + library_sources() + ["-ldl", "-o", str(exe)],
                   check=True, timeout=900)


def build_host_sanitized(harness, exe, sources=(), flags=()):
    """Compiles `harness` (a file of tests/native/) with g++ alone into the program `exe` under ASan + UBSan:
    a host-only program over the headers of csrc/, with `sources` (paths) compiled in and `flags` after them."""
    subprocess.run(["g++"] + SANITIZE + ["-fno-omit-frame-pointer", "-std=c++17", "-I" + CSRC,
                                         os.path.join(ROOT, "tests", "native", harness), *sources, *flags,
                                         "-o", str(exe)], check=True, timeout=300)


def run_harness(exe, args=(), timeout=600, env=None) -> str:
    """Runs a built harness; its output, after checking that it ended with status 0 (a sanitizer report does not)."""
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout
