"""GPU parity for ambrycrc_rekey_messages_dev against the oracle (tests/rekey_oracle.py: oracle/message_format.py
and zlib) and against the CPU entry: status, out_off, out_len and every output byte. The region and the output
each sit inside a larger tensor with 64 guard bytes of 0xA5 on both sides, which must survive."""
import functools

import numpy as np
import pytest

import rekey_oracle as RK
from datagen import stream_bytes
from gpu_buffers import assert_guards, guarded, guarded_workspace, guards_intact
from gpu_calls import assert_rekey_outputs, run_rekey
from msgfmt import MF
from regions import join, refused_messages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def messages(gpu):
    from ambry_amd import messages as M

    assert M.REKEY_DESC_DTYPE == RK.DESC
    return M


@functools.lru_cache(maxsize=None)
def case(seed):
    region, offs, meta = RK.build_region(n=300, seed=seed)
    descs, aux = RK.build_descs(offs, meta, seed=seed)
    return region, offs, descs, aux, RK.expected(region, offs, descs, aux)


@pytest.mark.parametrize("shift,oshift", [(0, 0), (1, 7), (13, 0), (63, 7)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_region_matches_oracle_and_cpu(messages, seed, shift, oshift):
    """Every stored format (headers V1-V3, SerDe V1-V5, blob records V1-V3, metadata blobs, update messages,
    10 % corrupted, blobs up to 300 KB: copies split across waves), the region at four offsets from a 64-B
    boundary and the output at two."""
    region, offs, descs, aux, exp = case(seed)
    RK.assert_mix(descs, exp[0])
    got = run_rekey(messages, region, offs, descs, aux, shift, oshift)
    assert_rekey_outputs(got, exp)
    if shift == 0:
        cst, couts = RK.run_cpu(messages, region, offs, descs, aux)
        assert cst == got[0]
        for b, o, n in zip(couts, got[1], got[2]):
            assert (b or b"") == got[3][o:o + n].tobytes() if n else not b


@functools.lru_cache(maxsize=None)
def exact_case(m):
    """m small messages of every stored format, 10 % corrupted, their descriptors and the oracle's answers."""
    region, offs, meta = RK.build_region(n=m, seed=800 + m, corrupt_frac=0.1 if m > 1 else 0.0, big_every=10**9,
                                         max_blob=600, max_usermeta=300)
    descs, aux = RK.build_descs(offs, meta, seed=800 + m)
    return region, offs, descs, aux, RK.expected(region, offs, descs, aux)


@pytest.mark.parametrize("m", [1, 512, 513])
def test_exact_workspace_between_guards(messages, m):
    """A caller workspace of exactly ambrycrc_rekey_workspace_bytes(m) between two guards, 0xA5 throughout: one
    message, and the counts on either side of one plan block (4 copy jobs a message: 2,048 / 2,052 jobs).
    Status, placement and every output byte as the oracle's; the workspace's guards intact."""

    region, offs, descs, aux, exp = exact_case(m)
    if m > 1:
        RK.assert_mix(descs, exp[0])
    whole, ws = guarded_workspace(messages.rekey_workspace_bytes(m))
    got = run_rekey(messages, region, offs, descs, aux, shift=13, oshift=7, workspace=ws)
    assert_guards(whole, ws)
    assert_rekey_outputs(got, exp)


@pytest.mark.parametrize("version", [1, 2])
def test_header_versions_and_life(messages, version):
    region, offs, descs, aux, _ = case(2)
    life = [(7 * i) % 32768 for i in range(len(offs))]
    exp = RK.expected(region, offs, descs, aux, life=life, version=version)
    RK.assert_mix(descs, exp[0])
    assert_rekey_outputs(run_rekey(messages, region, offs, descs, aux, shift=3, oshift=1, life=life, version=version), exp)


def test_no_room_advances_the_running_offset(messages):
    region, offs, descs, aux, full = case(3)
    cap = sum(full[2]) // 2 + 1
    exp = RK.expected(region, offs, descs, aux, out_cap=cap)
    refused = sum(1 for s in exp[0] if s == RK.NO_ROOM)
    assert 50 <= refused and any(n for n in exp[2])
    assert_rekey_outputs(run_rekey(messages, region, offs, descs, aux, shift=1, oshift=3, out_cap=cap), exp)


def test_replacement_content_sizes(messages):
    """Replacement contents of 0, 1, 63, 64, 65, 4096 and 70,000 bytes: the batch engine's tail and run
    boundaries and one job that splits across waves; each CRC extended over the 13-B head by a shift."""
    region, offs, descs, aux = RK.metadata_region([0, 1, 63, 64, 65, 4096, 70000])
    exp = RK.expected(region, offs, descs, aux)
    assert exp[0] == [0] * 7
    for version, oshift in ((3, 0), (1, 9)):
        exp = RK.expected(region, offs, descs, aux, version=version)
        got = run_rekey(messages, region, offs, descs, aux, shift=2, oshift=oshift, version=version)
        assert_rekey_outputs(got, exp)
        for o, n in zip(got[1], got[2]):
            assert MF.verify_message(got[3][o:o + n].tobytes(), 0) == (0, n)


def test_single_message_and_one_past_a_block(messages):
    region, offs, descs, aux, exp = case(1)
    i = next(k for k, s in enumerate(exp[0]) if s == 0 and exp[2][k])
    one = RK.expected(region, [offs[i]], descs[i:i + 1], aux)
    assert one[0] == [0]
    assert_rekey_outputs(run_rekey(messages, region, [offs[i]], descs[i:i + 1], aux, shift=9), one)
    # m = 257: small clean messages, one past a 256-thread block
    msgs = [RK.stored_put(MF.store_key("b%d" % k), MF.blob_properties_bytes(k, serde_version=1 + k % 5), b"u" * (k % 7),
                          stream_bytes(400 + k, 0, k).tobytes(), hv=1 + k % 3, bv=1 + k % 3) for k in range(257)]
    offs2 = [int(x) for x in np.cumsum([0] + [len(x) for x in msgs[:-1]])]
    descs2, aux2 = RK.build_descs(offs2, [False] * 257, seed=8, skip_frac=0.0, bad_frac=0.0)
    exp2 = RK.expected(b"".join(msgs), offs2, descs2, aux2)
    assert exp2[0] == [0] * 257
    assert_rekey_outputs(run_rekey(messages, b"".join(msgs), offs2, descs2, aux2, shift=5, oshift=2), exp2)


def test_all_refused_and_all_skipped_write_nothing(messages):
    region, offs, descs, aux, exp = case(2)
    bad = [i for i, s in enumerate(exp[0]) if s != 0][:40]
    assert len({exp[0][i] for i in bad}) >= 4
    st, off, ln, out = run_rekey(messages, region, [offs[i] for i in bad], descs[bad], aux, shift=1, oshift=1)
    assert st == [exp[0][i] for i in bad] and ln == [0] * len(bad) and off == [RK.NOWHERE] * len(bad)
    assert (out == 0xA5).all()
    skip = descs[:50].copy()
    skip["key_len"] = 0
    st, off, ln, out = run_rekey(messages, region, offs[:50], skip, aux, oshift=4)
    assert st == [0] * 50 and ln == [0] * 50 and off == [RK.NOWHERE] * 50
    assert (out == 0xA5).all()


@functools.lru_cache(maxsize=None)
def small_stored_puts():
    """300 clean stored PUTs with blobs under 1 KiB: headers V1..V3, SerDe V1..V5, blob records V1..V3, every
    other V2 / V3 one with an encryption key."""
    out = []
    for k in range(300):
        n = (k * 131) % 1024
        out.append(RK.stored_put(MF.store_key("s%d" % k), MF.blob_properties_bytes(n, serde_version=1 + k % 5),
                                 b"u" * (k % 7), stream_bytes(400 + k, 0, n).tobytes(), hv=1 + k % 3, bv=1 + k % 3,
                                 enc_key=b"e" * (1 + k % 40) if k % 2 else None))
    return out


@pytest.mark.parametrize("where", ["start", "middle", "end"])
@pytest.mark.parametrize("run", [40, 64, 200])
def test_runs_of_refused_messages(messages, run, where):
    """A run of consecutive messages the verify refuses (an update message, a wrong blob CRC, a wrong header CRC,
    by turns; every descriptor usable): rekey_write_kernel leaves each of them four copy jobs of cost 0, so with
    the jobs slot-major every slot holds `run` empty jobs at one start. gather_copy_kernel reads jobs in windows
    of 64 from the job its share begins in and jumps from a window of empty jobs to the end of the run: 40 end
    inside the window after the one that reaches them, 64 can fill a window, 200 leave whole empty windows, so
    the jump is taken and must land on the first job after the run. At the start of the batch the search for the
    first share's job must skip the run; at the end the last slot's run starts at the total cost."""

    puts = small_stored_puts()
    bad = refused_messages(run, "r%d" % run)
    first = {"start": 0, "middle": 150, "end": len(puts)}[where]
    msgs = puts[:first] + bad + puts[first:]
    region, offs = join(msgs)
    descs, aux = RK.build_descs(offs, [False] * len(msgs), seed=9, skip_frac=0.0, bad_frac=0.0)
    exp = RK.expected(region, offs, descs, aux)
    est = exp[0]
    assert all(est[first:first + run]) and sum(1 for s in est if s) == run
    assert len(set(est[first:first + run])) == 3
    got = run_rekey(messages, region, offs, descs, aux, shift=1, oshift=7)
    assert_rekey_outputs(got, exp)
    cst, couts = RK.run_cpu(messages, region, offs, descs, aux)
    assert cst == got[0]
    for b, o, n in zip(couts, got[1], got[2]):
        assert (b or b"") == got[3][o:o + n].tobytes() if n else not b


def test_graph_capture_and_replay(messages):
    """The call only enqueues work, so with a caller workspace it can be captured into a HIP graph and replayed
    on fresh data, with the outputs of the uncaptured call."""
    import torch

    region, offs, descs, aux, exp = case(1)
    rw, r = guarded(region, 0)
    aw, a = guarded(aux, 5)
    cap = messages.rekey_out_bound(len(region), len(offs), len(aux))
    ow, o = guarded(b"", 3, cap)
    fresh_r, fresh_o = rw.clone(), ow.clone()
    mo = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    dd = torch.from_numpy(np.ascontiguousarray(descs).view(np.uint8).reshape(-1).copy()).cuda()
    ws = torch.empty(messages.rekey_workspace_bytes(len(offs)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _, off0, len0, st0 = messages.rekey_dev(r, mo, dd, a, out=o, workspace=ws)  # loads the kernels outside the capture
        torch.cuda.synchronize()
        plain = (st0.cpu().numpy().view(np.uint32).tolist(), off0.cpu().numpy().view(np.uint64).tolist(),
                 len0.cpu().numpy().view(np.uint64).tolist(), guards_intact(ow, 3, cap).copy())
        assert_rekey_outputs(plain, exp)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _, off, ln, st = messages.rekey_dev(r, mo, dd, a, out=o, workspace=ws)
    torch.cuda.synchronize()
    for _ in range(2):
        rw.copy_(fresh_r)
        ow.copy_(fresh_o)
        st.zero_()
        ln.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (st.cpu().numpy().view(np.uint32).tolist(), off.cpu().numpy().view(np.uint64).tolist(),
               ln.cpu().numpy().view(np.uint64).tolist(), guards_intact(ow, 3, cap))
        assert_rekey_outputs(got, exp)
        assert got[:3] == plain[:3]
