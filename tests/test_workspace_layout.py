"""The device workspaces' sizes and layouts, on the CPU (the library loads without a device).

Every public *_workspace_bytes function is a workspace description run over null (csrc/ws_layout.h). Their
values are part of the ABI -- a caller sizes its buffer by them -- so they are pinned to a recorded table;
the descriptions themselves are walked by a stand-alone program under ASan + UBSan."""
import shutil

import pytest

import native_build
from workspace_sizes import M_VALUES, recorded

REGION_LENS = [0, 1, 4096, (1 << 20) + 1, 1 << 30]
OF_M = ["ambrycrc_workspace_bytes", "ambrycrc_messages_workspace_bytes", "ambrycrc_serialize_puts_workspace_bytes",
        "ambrycrc_transform_workspace_bytes", "ambrycrc_rekey_workspace_bytes", "ambrycrc_send_workspace_bytes",
        "ambrycrc_hard_delete_workspace_bytes", "ambrycrc_trailed_workspace_bytes"]
OF_REGION_M = ["ambrycrc_chain_workspace_bytes", "ambrycrc_recover_workspace_bytes"]


def size_table(lib):
    """{function: {argument(s): bytes}} of every public workspace size function at the recorded arguments."""
    t = {f: {str(m): getattr(lib, f)(m) for m in M_VALUES} for f in OF_M}
    for f in OF_REGION_M:
        t[f] = {f"{r},{m}": getattr(lib, f)(r, m) for r in REGION_LENS for m in M_VALUES}
    return t


def test_every_size_function_is_recorded(ambry):
    """The table covers every *_workspace_bytes symbol the binding declares."""
    from ambry_amd import _lib

    assert sorted(OF_M + OF_REGION_M) == sorted(n for n in _lib.EXPORTED if n.endswith("workspace_bytes"))


def test_workspace_sizes_match_the_recorded_table(ambry):
    """Exactly the values recorded from the library before the sizes were derived from the descriptions."""
    want = recorded("workspace_bytes")
    got = size_table(ambry.lib())
    assert sorted(got) == sorted(want)
    for fn in want:
        assert got[fn] == want[fn], fn


def test_layouts_under_asan(tmp_path):
    """tests/native/ws_layout_asan.cpp, host only, under ASan + UBSan: every description measured, carved over
    exactly that many malloc'd bytes and written end to end; arrays aligned, disjoint, inside the buffer."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "ws_layout_asan"
    native_build.build_host_sanitized("ws_layout_asan.cpp", exe, flags=native_build.HIP_HEADERS)
    out = native_build.run_harness(exe, timeout=300)
    assert "layouts=" in out and "bad=0" in out
