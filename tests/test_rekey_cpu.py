"""ambrycrc_rekey_message_cpu against the oracle (tests/rekey_oracle.py: oracle/message_format.py and zlib):
status and every output byte over regions of every stored format, the identity re-key against
MF.transform_message, the output capacity, the three header versions, and the entry under ASan + UBSan."""
import functools

import numpy as np
import pytest

import rekey_oracle as RK
from msgfmt import MF

SEEDS = [1, 2, 3]


@pytest.fixture(scope="module")
def messages(ambry):
    from ambry_amd import messages as M

    assert M.REKEY_DESC_DTYPE == RK.DESC
    assert (M.MSG_NEEDS_CONTENT, M.MSG_BAD_DESC, M.REKEY_KEEP) == (RK.NEEDS_CONTENT, RK.BAD_DESC, RK.KEEP)
    return M


@functools.lru_cache(maxsize=None)
def case(seed):
    region, offs, meta = RK.build_region(n=300, seed=seed)
    descs, aux = RK.build_descs(offs, meta, seed=seed)
    return region, offs, descs, aux


@pytest.mark.parametrize("seed", SEEDS)
def test_region_matches_oracle(messages, seed):
    region, offs, descs, aux = case(seed)
    est, _, _, _ = RK.expected(region, offs, descs, aux)
    RK.assert_mix(descs, est)
    eout = [RK.rekey_message(region, o, descs[i], aux)[1] for i, o in enumerate(offs)]
    st, outs = RK.run_cpu(messages, region, offs, descs, aux)
    assert st == est
    assert outs == eout
    # every re-keyed message verifies clean, under its new key
    for i, b in enumerate(outs):
        if b:
            assert MF.verify_message(b, 0) == (0, len(b))
            h = MF.HEADER_SIZE[3]
            assert b[h:h + int(descs[i]["key_len"])] == aux[int(descs[i]["key_src"]):][:int(descs[i]["key_len"])]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("version", [1, 2, 3])
def test_header_versions_and_life(messages, seed, version):
    region, offs, descs, aux = case(seed)
    life = [(7 * i) % 32768 for i in range(len(offs))]
    est = [RK.rekey_message(region, o, descs[i], aux, life[i], version) for i, o in enumerate(offs)]
    RK.assert_mix(descs, [s for s, _ in est])
    st, outs = RK.run_cpu(messages, region, offs, descs, aux, life=life, version=version)
    assert st == [s for s, _ in est]
    assert outs == [b for _, b in est]


@pytest.mark.parametrize("seed", SEEDS)
def test_identity_rekey_is_the_transform(messages, seed):
    """Re-keying with the stored key, the stored account / container and no content override gives
    MF.transform_message's bytes for every DataBlob message (and refuses what the transform refuses)."""
    region, offs, _, _ = case(seed)
    descs, aux = RK.identity_descs(region, offs)
    st, outs = RK.run_cpu(messages, region, offs, descs, aux)
    same = 0
    for i, off in enumerate(offs):
        tst, tb = MF.transform_message(region, off)
        if tst == 0 and RK.blob_type_of(region, off) == 1:
            assert st[i] == RK.NEEDS_CONTENT and outs[i] is None
            continue
        assert st[i] == tst and outs[i] == tb
        same += tst == 0
    assert same >= 180


def test_replacement_content_sizes(messages):
    """Metadata blobs stored at headers V1..V3 and blob records V2 / V3, replacement contents from empty to
    70,000 bytes, every output header version."""
    region, offs, descs, aux = RK.metadata_region([0, 1, 63, 64, 65, 4096, 70000])
    for version in (1, 2, 3):
        est = [RK.rekey_message(region, o, descs[i], aux, None, version) for i, o in enumerate(offs)]
        assert [s for s, _ in est] == [0] * 7
        st, outs = RK.run_cpu(messages, region, offs, descs, aux, version=version)
        assert st == [0] * 7 and outs == [b for _, b in est]
        for i, b in enumerate(outs):
            assert MF.verify_message(b, 0) == (0, len(b))
            assert b.count(aux[int(descs[i]["content_src"]):][:int(descs[i]["content_len"])]) >= 1


def test_out_cap_exact_and_one_short(messages):
    region, offs, descs, aux = case(1)
    buf, ax = np.frombuffer(region, dtype=np.uint8), np.frombuffer(aux, dtype=np.uint8)
    tried = 0
    for i, off in enumerate(offs[:60]):
        st, b = RK.rekey_message(region, off, descs[i], aux)
        if st or not b:
            continue
        assert messages.rekey_message_cpu(buf, off, descs[i], ax, out_cap=len(b)) == (0, b)
        assert messages.rekey_message_cpu(buf, off, descs[i], ax, out_cap=len(b) - 1) == (RK.NO_ROOM, None)
        tried += 1
    assert tried >= 30


def test_out_bound_is_enough(messages):
    """ambrycrc_rekey_out_bound never yields NO_ROOM: region + 26 B a message + aux, saturating."""
    region, offs, descs, aux = case(2)
    _, _, olen, packed = RK.expected(region, offs, descs, aux)
    assert len(packed) == sum(olen) <= messages.rekey_out_bound(len(region), len(offs), len(aux))
    assert messages.rekey_out_bound(10, 3, 5) == 10 + 3 * 26 + 5
    assert messages.rekey_out_bound(2**64 - 10, 1, 0) == 2**64 - 1 == messages.rekey_out_bound(0, 0, 2**64 - 1)
    assert messages.rekey_out_bound(2**63, 0, 2**63) == 2**64 - 1


def test_offsets_past_the_region_and_bad_arguments(messages):
    region, offs, descs, aux = case(3)
    buf, ax = np.frombuffer(region, dtype=np.uint8), np.frombuffer(aux, dtype=np.uint8)
    d = next(x for x in descs if int(x["key_len"]) and RK.desc_ok(x, len(aux)))
    for off in (len(region), len(region) + 1, len(region) - 1, 2**63):
        assert messages.rekey_message_cpu(buf, off, d, ax) == (MF.BAD_LAYOUT, None)
    skip = d.copy()
    skip["key_len"] = 0
    assert messages.rekey_message_cpu(buf, 2**63, skip, ax) == (0, b"")  # skipped: not read
    from ambry_amd import AmbryCrcError

    for version in (0, 4):
        with pytest.raises(AmbryCrcError):
            messages.rekey_message_cpu(buf, offs[0], d, ax, header_version=version)


def test_device_entry_checks_its_arguments_first(messages):
    """ambrycrc_rekey_messages_dev validates as the transform does, before it touches any memory: EINVAL for a
    null pointer, a header version outside 1..3, or aux bytes without a buffer; ENOINIT without a device
    context (no GPU is initialised in this process); m = 0 is a no-op. The workspace covers the verify's."""
    import ctypes

    from ambry_amd import lib
    from ambry_amd._lib import AMBRYCRC_EINVAL, AMBRYCRC_ENOINIT

    L = lib()
    p = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(256)))

    def call(region=p, offs=p, descs=p, aux=p, aux_len=8, hv=3, out=p, out_len=p, status=p, m=1):
        return L.ambrycrc_rekey_messages_dev(region, 64, offs, m, descs, aux, aux_len, None, hv, out, 64, None,
                                             out_len, status, None, 0, None)

    assert call(m=0) == 0
    for bad in ({"region": None}, {"offs": None}, {"descs": None}, {"out": None}, {"out_len": None},
                {"status": None}, {"aux": None}, {"hv": 0}, {"hv": 4}):
        assert call(**bad) == AMBRYCRC_EINVAL, bad
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        assert call() == AMBRYCRC_ENOINIT
        assert call(aux=None, aux_len=0) == AMBRYCRC_ENOINIT  # no aux at all is allowed
    for m in (1, 257, 100000):
        assert messages.rekey_workspace_bytes(m) >= L.ambrycrc_messages_workspace_bytes(m) + 264 * m


def test_rekey_cpu_under_asan(tmp_path):
    """The CPU entry parses untrusted bytes and untrusted descriptors: built with ASan + UBSan (host side) into
    a stand-alone program (tests/native/rekey_asan.cpp) that runs it over every message of a corrupted region,
    every tail truncation of the region, and descriptors whose spans touch both ends of aux or pass them,
    each time into an exactly sized heap buffer."""
    import subprocess

    import native_build

    if not native_build.have_toolchain():
        pytest.skip("hipcc/g++ not available")
    region, offs, meta = RK.build_region(n=40, seed=11, corrupt_frac=0.3, big_every=10**9)
    descs, aux = RK.build_descs(offs, meta, seed=11, bad_frac=0.2)
    files = {"region.bin": region, "offs.bin": np.asarray(offs, dtype="<u8").tobytes(), "descs.bin": descs.tobytes(),
             "aux.bin": aux}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    exe = tmp_path / "rekey_asan"
    native_build.build_sanitized("rekey_asan.cpp", exe, tmp_path)
    out = native_build.run_harness(exe, [str(tmp_path / n) for n in files])
    assert "runs=" in out and "bad=0" in out
