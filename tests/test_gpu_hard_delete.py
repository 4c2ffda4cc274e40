"""GPU parity for ambrycrc_hard_delete_messages_dev against the oracle (tests/hard_delete_oracle.py:
oracle/message_format.py and zlib) and against the CPU entry: status, recovery info and every byte of the
region after the delete. Every region sits inside a larger tensor with 64 guard bytes of 0xA5 on both sides,
which must survive."""
import functools

import numpy as np
import pytest

import hard_delete_oracle as HD
from datagen import stream_bytes
from gpu_buffers import assert_guards, guarded, guarded_workspace, guards_intact
from gpu_calls import run_hard_delete
from msgfmt import MF
from regions import join, refused_messages, verify_region

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def corrupt_region(seed):
    region, offs, _ = verify_region(n=300, seed=seed, corrupt_frac=0.1, big_every=17)
    return region, offs, HD.hard_delete(region, offs)


@pytest.mark.parametrize("shift", [0, 1, 13, 63])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_region_matches_oracle_and_cpu(gpu, seed, shift):
    """PUTs of header V1/V2/V3 (blobs up to 300 KB: ranges split across waves) and update messages, 10 %
    corrupted, the region at several offsets from a 64-B boundary."""
    region, offs, (est, einfo, eout) = corrupt_region(seed)
    deleted, refused, not_put, other = HD.counts(region, offs, est)
    assert deleted >= 200 and refused >= 20 and not_put >= 20 and other >= 1, (deleted, refused, not_put, other)
    st, info, out = run_hard_delete(gpu, region, offs, shift)
    assert st == est
    assert np.array_equal(info, einfo)
    assert out == eout
    if shift == 0:
        assert (st, out) == HD.run_cpu(gpu, region, offs)[::2]


@functools.lru_cache(maxsize=None)
def exact_case(m):
    """m small messages, 10 % corrupted (build_region's first message, the one with a blob of 60 KB and more,
    left out), and the oracle's answers."""
    region, offs, _ = verify_region(n=m + 1, seed=700 + m, corrupt_frac=0.1 if m > 1 else 0.0, big_every=10**9)
    region, offs = region[offs[1]:], [o - offs[1] for o in offs[1:]]
    return region, offs, HD.hard_delete(region, offs)


@pytest.mark.parametrize("m", [1, 1024, 1025])
def test_exact_workspace_between_guards(gpu, m):
    """A caller workspace of exactly ambrycrc_hard_delete_workspace_bytes(m) between two guards, 0xA5
    throughout: one message, and the counts on either side of one plan block (2 jobs a message: 2,048 / 2,050
    jobs). Status, info and every region byte as the oracle's; the workspace's guards intact."""

    region, offs, (est, einfo, eout) = exact_case(m)
    deleted, refused, not_put, _ = HD.counts(region, offs, est)
    assert (deleted, refused, not_put) == (1, 0, 0) if m == 1 else deleted >= 700 and refused >= 50 and not_put >= 50
    whole, ws = guarded_workspace(gpu.hard_delete_workspace_bytes(m))
    st, info, out = run_hard_delete(gpu, region, offs, shift=13, workspace=ws)
    assert_guards(whole, ws)
    assert st == est
    assert np.array_equal(info, einfo)
    assert out == eout


def test_alignment_grid(gpu):
    """Messages packed back to back with key lengths 1..16, so the zero spans start on every residue mod 16,
    crossed with user-metadata and blob sizes around the 16-B piece and the 64-lane store."""
    msgs = []
    for klen in range(1, 17):
        for un in (0, 1, 15, 16, 17):
            for bn in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 4095, 4097):
                i = len(msgs)
                msgs.append(MF.put_message(MF.store_key("k" * klen), MF.blob_properties_bytes(bn),
                                           stream_bytes(500 + i, 0, un).tobytes() if un else b"",
                                           stream_bytes(9000 + i, 0, bn).tobytes() if bn else b"", version=1 + i % 3))
    region, offs = join(msgs)
    est, einfo, eout = HD.hard_delete(region, offs)
    assert {(o + int(r["start"]) + 6) % 16 for o, r in zip(offs, einfo)} == set(range(16))
    assert all(s == 0 for s in est)
    for shift in (0, 5):
        st, info, out = run_hard_delete(gpu, region, offs, shift)
        assert st == est and np.array_equal(info, einfo)
        assert out == eout


def test_share_boundaries(gpu):
    """One 4 MiB + 1 B blob and one 1 MiB - 3 B blob among 200 small messages: the long ranges are cut into
    many waves' shares, each with its own unaligned ends."""
    sizes = {37: (4 << 20) + 1, 150: (1 << 20) - 3}
    msgs = []
    for i in range(200):
        size = sizes.get(i, 50 + (i * 131) % 3000)
        msgs.append(MF.put_message(MF.store_key("S%d" % i), MF.blob_properties_bytes(size), b"u" * (i % 23),
                                   stream_bytes(7000 + i, 0, size).tobytes(), version=1 + i % 3))
    region, offs = join(msgs)
    est, einfo, eout = HD.hard_delete(region, offs)
    st, info, out = run_hard_delete(gpu, region, offs, shift=3)
    assert st == est == [0] * 200 and np.array_equal(info, einfo)
    assert out == eout


def test_two_phases(gpu):
    """HardDeleter's two phases (HardDeleter.java:655-700): plan_only leaves the region as it is and returns
    the recovery info; the second call with that info, on a copy whose blob bodies were damaged in between,
    deletes every PUT without reading the record CRCs; bad recovery fields are refused."""
    region, offs, _ = verify_region(n=300, seed=2, corrupt_frac=0.0, big_every=17)
    est, einfo, eout = HD.hard_delete(region, offs)
    st, info, out = run_hard_delete(gpu, region, offs, plan_only=True)
    assert st == est and np.array_equal(info, einfo) and out == region
    damaged, flipped = HD.flip_blob_bodies(region, offs, info)
    assert flipped >= 50
    st, _, out = run_hard_delete(gpu, damaged, offs)
    assert sum(1 for s in st if s == MF.BLOB_CRC) == flipped
    st, info2, out = run_hard_delete(gpu, damaged, offs, shift=7, recovery=info)
    assert st == est and np.array_equal(info2, einfo)
    assert out == eout
    # one bad field per message, by turns; messages left with good info are still deleted
    rec = info.copy()
    puts = [i for i in range(len(offs)) if int(info[i]["header_version"]) and int(info[i]["usermeta_size"])
            and int(info[i]["blob_size"])]
    for n, i in enumerate(puts[::2]):
        rec[i] = HD.bad_recoveries(info[i])[n % 7]
    exp = HD.hard_delete(region, offs, rec)
    assert sum(1 for s in exp[0] if s == MF.BAD_RECORD) == len(puts[::2])
    st, info3, out = run_hard_delete(gpu, region, offs, recovery=rec)
    assert st == exp[0] and np.array_equal(info3, exp[1])
    assert out == exp[2]


def test_deleted_messages_verify_clean(gpu):
    import torch

    region, offs, _ = verify_region(n=300, seed=3, corrupt_frac=0.0, big_every=17)
    whole, r = guarded(region)
    o = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    st, _ = gpu.hard_delete_messages(r, o)
    vst, _ = gpu.verify_messages(r, o)
    torch.cuda.synchronize()
    st = st.cpu().numpy().view(np.uint32)
    assert (st == 0).sum() >= 200 and set(st.tolist()) == {0, MF.NOT_PUT}
    assert (vst.cpu().numpy() == 0).all()
    assert guards_intact(whole, 0, len(region)).tobytes() == HD.hard_delete(region, offs)[2]


def test_duplicate_offset_empty_and_single(gpu):
    import torch

    region, offs, _ = verify_region(n=40, seed=6, corrupt_frac=0.1, big_every=10**9)
    twice = offs + [offs[3], offs[3], offs[20]] + [len(region) + 5, len(region) - 1]  # and two past the region's end
    est, einfo, eout = HD.hard_delete(region, twice)
    st, info, out = run_hard_delete(gpu, region, twice, shift=1)
    assert st == est and np.array_equal(info, einfo) and out == eout
    st, info, out = run_hard_delete(gpu, region, [])
    assert st == [] and len(info) == 0 and out == region
    put = next(o for o, s in zip(offs, est) if s == 0)
    st, info, out = run_hard_delete(gpu, region, [put])
    assert (st, out) == HD.hard_delete(region, [put])[::2] and st == [0]


@functools.lru_cache(maxsize=None)
def small_puts():
    """1,300 clean PUTs of at most 600 B of blob, header V1/V2/V3."""
    return [MF.put_message(MF.store_key("p%d" % i), MF.blob_properties_bytes((i * 131) % 600), b"m" * (i % 23),
                           stream_bytes(5000 + i, 0, (i * 131) % 600).tobytes(), version=1 + i % 3)
            for i in range(1300)]


@pytest.mark.parametrize("where", ["start", "middle", "end"])
@pytest.mark.parametrize("run", [40, 64, 200])
def test_runs_of_refused_messages(gpu, run, where):
    """A run of consecutive refused messages: two fill jobs each, of cost 0 and all at one start. hd_fill_kernel
    reads jobs in windows of 64, the first starting at the job its share begins in, and jumps from a window of
    empty jobs to the end of the run. Directly after a PUT with a 300 KB blob, the wave that finishes the blob
    walks into the run: 40 messages (80 jobs) end inside its second window, which still reaches work; 64 (128
    jobs) make that window empty and 200 (400 jobs) leave more empty windows behind it, so the jump is taken and
    must land on the first PUT after the run. At the very start of the batch the search for a share's first job
    must skip the run, and at the very end the run's jobs all start at the total cost."""
    puts = small_puts()
    bad = refused_messages(run, "r%d" % run)
    if where == "start":
        msgs, first = bad + puts, 0
    elif where == "end":
        msgs, first = puts + bad, len(puts)
    else:
        big = MF.put_message(MF.store_key("big"), MF.blob_properties_bytes(300_000), b"meta",
                             stream_bytes(77, 0, 300_000).tobytes(), version=3)
        msgs, first = puts[:650] + [big] + bad + puts[650:], 651
    region, offs = join(msgs)
    est, einfo, eout = HD.hard_delete(region, offs)
    assert all(est[first:first + run]) and sum(1 for s in est if s) == run
    assert len({s for s in est[first:first + run]}) == 3
    st, info, out = run_hard_delete(gpu, region, offs, shift=3)
    assert st == est
    assert np.array_equal(info, einfo)
    assert out == eout


def test_every_message_refused(gpu):
    """No message is deleted: no fill job has any cost, the region comes back byte for byte and every info entry
    is zero."""
    msgs = refused_messages(300, "none")
    region, offs = join(msgs)
    est, einfo, eout = HD.hard_delete(region, offs)
    assert all(est) and eout == region
    for plan_only in (False, True):
        st, info, out = run_hard_delete(gpu, region, offs, shift=1, plan_only=plan_only)
        assert st == est
        assert np.array_equal(info, np.zeros(len(offs), dtype=HD.INFO)) and np.array_equal(info, einfo)
        assert out == region


def test_graph_capture_and_replay(gpu):
    """The call only enqueues work, so with a caller workspace it can be captured into a HIP graph (a linear
    one) and replayed on a fresh copy of the region, byte-exact."""
    import torch

    region, offs, (est, einfo, eout) = corrupt_region(1)
    whole, r = guarded(region)
    fresh = whole.clone()
    o = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    ws = torch.empty(gpu.hard_delete_workspace_bytes(len(offs)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gpu.hard_delete_messages(r, o, workspace=ws)  # loads the kernels outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            st, info = gpu.hard_delete_messages(r, o, workspace=ws)
    torch.cuda.synchronize()
    for _ in range(2):
        whole.copy_(fresh)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert st.cpu().numpy().view(np.uint32).tolist() == est
        assert np.array_equal(info.cpu().numpy().reshape(-1).view(HD.INFO), einfo)
        assert guards_intact(whole, 0, len(region)).tobytes() == eout
