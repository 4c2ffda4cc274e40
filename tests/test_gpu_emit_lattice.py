"""Every device entry that writes a stored PUT message, over the writer lattice (tests/emit_lattice.py), against
the oracles test_emit_lattice.py holds the CPU entries to: so each equals its CPU twin. Each test is one call a
header version over one region."""
import numpy as np
import pytest

import emit_lattice as EL
import rekey_oracle as RK
from emit_lattice import OUT_VERSIONS, assert_packed, ingest_expected, rekey_expected, transform_expected
from gpu_buffers import dev
from gpu_calls import assert_ingest_outputs, assert_rekey_outputs, run_ingest, run_rekey
from msgfmt import MF

pytestmark = pytest.mark.gpu


def run_transform(gpu, region, offs, version, use_life):
    import torch

    from ambry_amd.messages import transform_dev

    life = (np.arange(len(offs)) % 5).astype(np.int16)
    out, oo, ol, st = transform_dev(dev(region), torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda"),
                                    header_version=version, life_version=torch.from_numpy(life).cuda() if use_life else None)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), oo.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_transform_general(gpu, version):
    region, offs, cs = EL.region()
    for use_life in (True, False):
        got = run_transform(gpu, region, offs, version, use_life)
        assert gpu.last_transform_path(0) == 0  # the lattice is not the fast path's dense run of canonical V3 PUTs
        assert_packed(*got, transform_expected(version, use_life), [c.name for c in cs])


def test_transform_fast(gpu):
    """The cases that qualify, as a dense run: the fast path takes the batch. With one more message it cannot take
    (a stored isCompressed byte other than 0 / 1, which the reference reads as false and writes as 0) the general
    path redoes the batch."""
    region, offs, cs = EL.fast_region()
    for use_life in (True, False):
        got = run_transform(gpu, region, offs, 3, use_life)
        assert gpu.last_transform_path(0) == 1
        assert_packed(*got, transform_expected(3, use_life, True), [c.name for c in cs])
    spoil = [c for c in EL.cases() if c.hv == 3 and c.bv == 3 and c.sv == 5 and c.comp == 2][0]
    region2, offs2 = region + spoil.stored(), offs + [len(region)]
    got = run_transform(gpu, region2, offs2, 3, False)
    assert gpu.last_transform_path(0) == 0
    assert_packed(*got, [MF.transform_message(region2, o, version=3) for o in offs2], [c.name for c in cs] + [spoil.name])


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_transform_host_gpu_leg(gpu, version):
    from ambry_amd import messages

    region, offs, cs = EL.region()
    life = (np.arange(len(offs)) % 5).astype(np.int16)
    out, oo, ol, st = messages.transform_host(region, offs, header_version=version, life_version=life)
    assert gpu.last_host_path(0) == 1
    assert_packed(out, oo, ol, st, transform_expected(version, True), [c.name for c in cs])


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_rekey(gpu, version):
    from ambry_amd import messages

    region, offs, cs = EL.region()
    descs, aux = EL.rekey_inputs()
    for life in (None, [i % 5 for i in range(len(offs))]):
        exp = RK.expected(region, offs, descs, aux, life=life, version=version)
        assert [(s, exp[3][o:o + n]) for s, o, n in zip(*exp[:3])] == rekey_expected(version, life is not None)
        assert_rekey_outputs(run_rekey(messages, region, offs, descs, aux, shift=5, oshift=3, life=life,
                                       version=version), exp)


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_ingest(gpu, version):
    from ambry_amd import messages

    wire, refs = EL.wire()
    assert_ingest_outputs(run_ingest(messages, wire, refs, shift=3, oshift=1, version=version),
                          ingest_expected(version))


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_serialize_copy_mode(gpu, version):
    """Copy mode with both sources: the streamed form for the lattice's messages, and (one message above its limit)
    the job path beside it."""
    import torch

    from ambry_amd import messages

    for big_tail in (False, True):
        msgs, exp = EL.put_messages(version, big_tail)
        descs, fields, blobs, offs, total = messages.pack_batch(msgs, gap=3)
        out = torch.full((total + 16,), 0xAA, dtype=torch.uint8, device="cuda")
        msg_len = torch.zeros(len(msgs), dtype=torch.int64, device="cuda")
        messages.serialize_dev(torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).cuda(), out, dev(fields),
                               dev(blobs), msg_len=msg_len)
        torch.cuda.synchronize()
        image = np.full(total + 16, 0xAA, dtype=np.uint8)
        for o, e in zip(offs, exp):
            image[o:o + len(e)] = np.frombuffer(e, dtype=np.uint8)
        got = out.cpu().numpy()
        bad = np.nonzero(got != image)[0]
        assert not len(bad), "first differing byte %d, in message %d" % (bad[0], np.searchsorted(offs, bad[0], "right") - 1)
        assert msg_len.cpu().tolist() == [len(e) for e in exp]
