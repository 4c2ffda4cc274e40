"""ambrycrc_send_message_cpu against the oracle (tests/send_oracle.py: oracle/message_format.py and zlib):
status, info and every sent byte over regions of every stored format under all five MessageFormatFlags,
each rule of the entry once, the output capacity, and the entry under ASan + UBSan."""
import functools

import numpy as np
import pytest

import rekey_oracle as RK
import send_oracle as SO
from msgfmt import MF
from oracle_common import same

FLAG_NAMES = {SO.BLOB_PROPERTIES: "props", SO.BLOB_USER_METADATA: "usermeta", SO.BLOB: "blob", SO.ALL: "all",
              SO.BLOB_INFO: "info"}


@pytest.fixture(scope="module")
def messages(ambry):
    from ambry_amd import messages as M

    assert M.SEND_INFO_DTYPE == SO.INFO
    assert (M.SEND_BLOB_PROPERTIES, M.SEND_BLOB_USER_METADATA, M.SEND_BLOB, M.SEND_ALL, M.SEND_BLOB_INFO) == SO.FLAGS
    assert M.SEND_NOWHERE == SO.NOWHERE and M.MSG_NO_ROOM == SO.NO_ROOM
    return M


@functools.lru_cache(maxsize=None)
def region_case(seed):
    region, offs, _ = RK.build_region(n=300, seed=seed)
    # readSet.sizeInBytes: the header's length where it parses, else up to the next message
    ends = offs[1:] + [len(region)]
    sizes = [SO.header_length(region, o) or e - o for o, e in zip(offs, ends)]
    return region, offs, sizes


@functools.lru_cache(maxsize=None)
def rules():
    return SO.rule_cases()


def assert_same(got, exp):
    gst, ginfo, gout = got
    est, einfo, eout = exp
    assert list(gst) == list(est)
    same(ginfo, einfo, "info")
    assert gout == eout


@pytest.mark.parametrize("flag", SO.FLAGS, ids=FLAG_NAMES.get)
@pytest.mark.parametrize("sized", [False, True], ids=["header-size", "given-size"])
def test_region_matches_oracle(messages, flag, sized):
    region, offs, sizes = region_case(1)
    exp = SO.expected(region, offs, sizes if sized else None, flag)
    clean, found, refused = SO.mix(exp[0], exp[1])
    assert clean >= 1 and found >= 1 and (refused >= 1 or (flag == SO.ALL and sized)), (clean, found, refused)
    assert_same(SO.run_cpu(messages, region, offs, sizes if sized else None, flag), exp)
    # what is sent is the stored bytes verbatim
    for i, f in enumerate(exp[1]):
        if exp[0][i] == 0:
            lo = offs[i] + int(f["rel_off"])
            assert exp[2][int(f["out_off"]):][:int(f["send_len"])] == region[lo:lo + int(f["send_len"])]


@pytest.mark.parametrize("flag", SO.FLAGS, ids=FLAG_NAMES.get)
@pytest.mark.parametrize("sized", [False, True], ids=["header-size", "given-size"])
def test_each_rule(messages, flag, sized):
    names, region, offs, sizes = rules()
    # the CPU entry's size 0 means "the header's": the batch's refusal of a size of 0 is a device test
    sz = [s or None for s in sizes] if sized else None
    buf = np.frombuffer(region, dtype=np.uint8)
    for i, name in enumerate(names):
        size = None if sz is None else sz[i]
        st, f, b = messages.send_message_cpu(buf, offs[i], flag, size=size)
        est, ef, eb = SO.send_message(region, offs[i], size, flag)
        assert st == est, name
        assert {n: int(f[n]) for n in SO.INFO.names} == ef, name
        assert b == eb, name
    by = {n: i for i, n in enumerate(names)}

    def one(name):
        i = by[name]
        return messages.send_message_cpu(buf, offs[i], flag, size=None if sz is None else sz[i])

    meta = flag in (SO.BLOB_PROPERTIES, SO.BLOB_USER_METADATA, SO.BLOB_INFO)
    # a flipped blob byte: counted under ALL and BLOB, never looked at under the metadata flags
    for name in ("v3-content", "v3-trailer", "v1-content"):
        st, f, b = one(name)
        assert st == 0 and int(f["check"]) == (0 if meta else MF.BLOB_CRC), name
        lo = offs[by[name]] + int(f["rel_off"])
        assert b == region[lo:lo + int(f["send_len"])]
    # the encryption-key record: fatal where deserializeBlobEncryptionKey runs, counted under ALL, unread under
    # BLOB_PROPERTIES
    for name, bit in (("v3-enckey", MF.ENCKEY_CRC), ("v3-enckey-version", MF.BAD_VERSION),
                      ("v3-enckey-size", MF.BAD_RECORD)):
        st, f, b = one(name)
        if flag == SO.ALL:
            assert st == 0 and int(f["check"]) == bit and b is not None
        elif flag == SO.BLOB_PROPERTIES:
            assert st == 0 and int(f["check"]) == 0 and int(f["enckey_rel"]) == 0
        else:
            assert st == bit and b is None and int(f["out_off"]) == SO.NOWHERE and int(f["send_len"]) == 0
    # a clean message with an encryption key reports where the key bytes are
    st, f, _ = one("v3-clean")
    rel0 = MF.parse_header(region, offs[by["v3-clean"]])[2][0]
    assert st == 0 and int(f["check"]) == 0
    assert (int(f["enckey_rel"]), int(f["enckey_len"])) == ((rel0 + 6, 32) if flag in (SO.BLOB, SO.BLOB_USER_METADATA,
                                                                                      SO.BLOB_INFO) else (0, 0))
    # the header: fatal, except under ALL with a size, where the message goes whole
    for name, bit in (("v3-header", MF.HEADER_CRC), ("v1-bad-version-sized", MF.BAD_VERSION)):
        st, f, b = one(name)
        i = by[name]
        if flag == SO.ALL and sized:
            assert st == 0 and int(f["check"]) == bit and b == region[offs[i]:offs[i] + sizes[i]]
        else:
            assert st == bit and b is None
    # an update message: sent under ALL with NOT_PUT counted, refused otherwise
    st, f, b = one("update")
    assert (st, int(f["check"])) == ((0, MF.NOT_PUT) if flag == SO.ALL else (MF.NOT_PUT, 0))
    # sizes
    if sized:
        assert one("past-region")[0] == MF.BAD_LAYOUT
        st, f, b = one("v3-smaller")
        if flag == SO.ALL:
            assert st == 0 and int(f["check"]) == MF.BAD_LAYOUT and len(b) == sizes[by["v3-smaller"]]
        else:
            assert st == (MF.BAD_LAYOUT if flag == SO.BLOB else 0)
        st, f, b = one("v3-larger")
        assert st == 0 and int(f["check"]) == 0 and (flag != SO.ALL or len(b) == sizes[by["v3-larger"]])
        assert one("v3-much-smaller")[0] == (0 if flag in (SO.ALL, SO.BLOB_PROPERTIES) else MF.BAD_LAYOUT)


@pytest.mark.parametrize("flag", SO.FLAGS, ids=FLAG_NAMES.get)
def test_out_cap_at_half_the_total(messages, flag):
    region, offs, sizes = region_case(2)
    total = len(SO.expected(region, offs, None, flag)[2])
    exp = SO.expected(region, offs, None, flag, out_cap=total // 2)
    assert sum(1 for s in exp[0] if s == SO.NO_ROOM) >= 20 and len(exp[2]) <= total // 2
    assert_same(SO.run_cpu(messages, region, offs, None, flag, out_cap=total // 2), exp)
    # exactly its length fits, one byte less does not
    buf = np.frombuffer(region, dtype=np.uint8)
    i = next(i for i, s in enumerate(exp[0]) if s == 0)
    n = int(exp[1][i]["send_len"])
    assert messages.send_message_cpu(buf, offs[i], flag, out_cap=n)[0] == 0
    assert messages.send_message_cpu(buf, offs[i], flag, out_cap=n - 1)[0] == SO.NO_ROOM


def test_bad_arguments(messages):
    import ctypes

    from ambry_amd import AmbryCrcError, lib
    from ambry_amd._lib import AMBRYCRC_EINVAL

    region, offs, _ = region_case(1)
    buf = np.frombuffer(region, dtype=np.uint8)
    for flag in (-1, 5):
        with pytest.raises(AmbryCrcError):
            messages.send_message_cpu(buf, offs[0], flag)
    for off in (len(region), len(region) + 1, 2**63):
        assert messages.send_message_cpu(buf, off, SO.BLOB)[0] == MF.BAD_LAYOUT
    L = lib()
    p = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(256)))

    def call(region=p, offs=p, out=p, info=p, status=p, flag=SO.BLOB, m=1):
        return L.ambrycrc_send_messages_dev(region, 64, offs, None, m, flag, out, 64, info, status, None, 0, None)

    assert call(m=0) == 0
    for bad in ({"region": None}, {"offs": None}, {"out": None}, {"info": None}, {"status": None}, {"flag": 5},
                {"flag": -1}):
        assert call(**bad) == AMBRYCRC_EINVAL, bad
    for m in (1, 257, 100000):
        assert messages.send_workspace_bytes(m) >= L.ambrycrc_messages_workspace_bytes(m) + 100 * m


def test_send_cpu_under_asan(tmp_path):
    """The CPU entry parses untrusted bytes: built with ASan + UBSan (host side) into a stand-alone program
    (tests/native/send_asan.cpp) that runs it over the rule cases and a corrupted region, every flag, with and
    without a size, every message as an exactly sized heap copy, and on every tail truncation."""
    import subprocess

    import native_build

    if not native_build.have_toolchain():
        pytest.skip("hipcc/g++ not available")
    region, offs, _ = RK.build_region(n=40, seed=11, corrupt_frac=0.3, big_every=10**9)
    _, rregion, roffs, _ = rules()
    files = {"region.bin": region, "offs.bin": np.asarray(offs, dtype="<u8").tobytes(),
             "rules.bin": rregion, "roffs.bin": np.asarray(roffs, dtype="<u8").tobytes()}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    exe = tmp_path / "send_asan"
    native_build.build_sanitized("send_asan.cpp", exe, tmp_path)
    out = native_build.run_harness(exe, [str(tmp_path / n) for n in files])
    assert "runs=" in out and "bad=0" in out
