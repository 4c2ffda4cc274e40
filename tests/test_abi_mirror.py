"""ambry_amd/abi.py against include/ambrycrc.h itself: a C program generated from the header's text (its struct,
field and macro names taken by regex, none retyped here) prints every struct's size, every field's offset and
size and every numeric macro's value; the mirrors must say the same."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ambry_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ambrycrc.h")
UINT64_MAX = (1 << 64) - 1


def parse_header():
    """({struct: [field, ...]}, [numeric macro, ...]) of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    structs = {}
    for name, body in re.findall(r"typedef struct (ambrycrc_\w+) \{(.*?)\}\s*\1;", text, flags=re.S):
        decls = [d.strip() for d in body.split(";") if d.strip()]
        structs[name] = [re.search(r"(\w+)\s*(\[\d+\])?$", part.strip()).group(1)
                         for d in decls for part in d.split(",")]
    macros = [m for m, value in re.findall(r"^#define (AMBRYCRC_\w+)[ \t]+(\S.*?)\s*$", text, flags=re.M)
              if re.fullmatch(r"[-()\s\dxXa-fA-Fu<]+", value)]
    return structs, macros


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """What the compiled header says: ({struct: (size, [(field, offset, size), ...])}, {macro: value})."""
    structs, macros = parse_header()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ambrycrc.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f)
                  for f in fields]
    lines += ['  printf("M %s %%lld\\n", (long long)(%s));' % (m, m) for m in macros]
    tmp = tmp_path_factory.mktemp("abi_mirror")
    src, exe = str(tmp / "mirror.c"), str(tmp / "mirror")
    with open(src, "w") as f:
        f.write("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", "-o", exe, src], check=True, capture_output=True)
    sizes, fields, values = {}, {}, {}
    for kind, *rest in (line.split() for line in subprocess.run([exe], check=True, capture_output=True,
                                                                text=True).stdout.splitlines()):
        if kind == "S":
            sizes[rest[0]] = int(rest[1])
        elif kind == "F":
            fields.setdefault(rest[0], []).append((rest[1], int(rest[2]), int(rest[3])))
        else:
            values[rest[0]] = int(rest[1])
    return {s: (sizes[s], fields[s]) for s in sizes}, values


def mirror_layout(mirror):
    """(size, [(field, offset, size), ...]) of a numpy dtype or a ctypes structure."""
    if isinstance(mirror, np.dtype):
        return mirror.itemsize, [(n, mirror.fields[n][1], mirror.fields[n][0].itemsize) for n in mirror.names]
    return ctypes.sizeof(mirror), [(n, getattr(mirror, n).offset, getattr(mirror, n).size) for n, _ in mirror._fields_]


def test_every_struct_has_the_headers_layout(header):
    structs, _ = header
    assert len(structs) == 9 and {"ambrycrc_" + s for s in abi.STRUCTS} == set(structs)
    for name, mirror in abi.STRUCTS.items():
        assert mirror_layout(mirror) == structs["ambrycrc_" + name], name
    assert mirror_layout(abi.PUT_DESC_DTYPE) == structs["ambrycrc_put_desc"]  # the derived twin of PutDesc


def python_name(macro):
    """AMBRYCRC_X is X in abi.py, except the error codes, which keep the whole name."""
    return macro if hasattr(abi, macro) else macro[len("AMBRYCRC_"):]


def test_every_constant_has_the_headers_value(header):
    _, values = header
    assert len(values) >= 33  # 8 error codes, 17 status bits, 5 flags, 3 sizes
    for macro, value in values.items():
        assert getattr(abi, python_name(macro), None) == value, macro
    for bit in (*range(0, 6), *range(8, 19)):
        assert (1 << bit) in [v for m, v in values.items() if m.startswith("AMBRYCRC_MSG_")], bit


def test_no_constant_the_header_lacks(header):
    """Every MSG_* / SEND_* / AMBRYCRC_* name of abi.py is a macro of the header (the sentinels, all UINT64_MAX,
    are the header's comments, not its macros)."""
    _, values = header
    known = {python_name(m) for m in values}
    for name, value in vars(abi).items():
        if name.startswith(("MSG_", "SEND_", "AMBRYCRC_")) and isinstance(value, int) and value != UINT64_MAX:
            assert name in known, name
    assert abi.REKEY_KEEP == abi.SEND_NOWHERE == abi.RECV_NOWHERE == abi.RECV_TO_END == abi.NO_MESSAGE == UINT64_MAX


def test_reexports_are_the_same_objects():
    from ambry_amd import _lib
    from ambry_amd import device as D
    from ambry_amd import messages as M

    assert _lib.PutDesc is abi.PutDesc and _lib.Shard is abi.Shard and _lib.AMBRYCRC_EPROBE == abi.AMBRYCRC_EPROBE
    assert M.PUT_DESC_DTYPE is abi.PUT_DESC_DTYPE and M.MSG_NO_ROOM == abi.MSG_NO_ROOM and M.SEND_ALL == abi.SEND_ALL
    assert D.HARD_DELETE_INFO is abi.HARD_DELETE_INFO and D.MESSAGE_INFO is abi.MESSAGE_INFO
    assert D.RECOVER_RESULT is abi.RECOVER_RESULT and D.MSG_BAD_INFO == abi.MSG_BAD_INFO
