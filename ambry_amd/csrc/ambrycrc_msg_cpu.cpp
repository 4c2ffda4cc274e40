// ambrycrc_msg_cpu.cpp -- one stored message on the CPU: deserializeBlobAll's checks
// (MessageFormatRecord.java:257-303) and ValidatingTransformer.transform
// (ValidatingTransformer.java:46-104), for the per-message callers (a GET of one blob, a
// replication thread transforming one message) that a device batch does not fit. The
// semantics and status bits are ambrycrc_verify_messages_dev's and
// ambrycrc_transform_messages_dev's (message_kernels.hip); the CRCs run through the CLMUL
// host loop (ambrycrc_update).
#include "../../include/ambrycrc.h"

#include <string.h>

#include "hard_delete.h"
#include "msg_header.h"
#include "put_emit.h"
#include "put_layout.h"
#include "record_fields.h"
#include "recover.h"
#include "rekey.h"
#include "send.h"

namespace {

using ambrycrc::ld_be16;
using ambrycrc::ld_be32;
using ambrycrc::ld_be64;
using ambrycrc::record_check;

constexpr uint32_t kRecordBit[ambrycrc::kMsgSlots] = {AMBRYCRC_MSG_ENCKEY_CRC, AMBRYCRC_MSG_PROPS_CRC, AMBRYCRC_MSG_UPDATE_CRC,
                                    AMBRYCRC_MSG_USERMETA_CRC, AMBRYCRC_MSG_BLOB_CRC};

// msg_header.h's field source and CRC for a header in host memory (the CLMUL loop).
struct HostCrc {
  const uint8_t* p;
  uint32_t operator()(uint32_t n) const { return ambrycrc_update(0, p, n); }
};
uint32_t decode(const uint8_t* p, uint64_t rem, ambrycrc::MsgHeader* H) {
  return ambrycrc::msg_decode(ambrycrc::HeaderBytes{p}, rem, HostCrc{p}, H);
}

// Header and every record of the message at p (rem bytes available): status bits; *end the message
// end relative to p, 0 when the header is refused.
uint32_t verify(const uint8_t* p, uint64_t rem, ambrycrc::MsgHeader* H, uint64_t* end) {
  *end = 0;
  ambrycrc::MsgLayout L;
  uint32_t status = decode(p, rem, H);
  if (status == 0) status = ambrycrc::msg_layout(*H, rem, &L);
  if (status) return status;
  for (int k = 0; k < ambrycrc::kMsgSlots; ++k) {
    if (L.rel[k] == -1) continue;
    const uint8_t* q = p + L.rel[k];
    const uint64_t span = L.rend[k] - (uint64_t)L.rel[k];
    if ((uint64_t)ambrycrc_update(0, q, span - 8) != ld_be64(q + span - 8)) status |= kRecordBit[k];
    status |= record_check(k, q, span);
  }
  *end = L.end;
  return status;
}

// ValidatingTransformer.transform of one message, split for the batch: transform_plan verifies the
// message and decides its output (status, length, and how to write it) without writing; transform_emit
// writes it. The batch plans every message, places them by one prefix sum and emits each straight
// into the output, with no scratch copy.
struct XPlan {
  uint64_t len = 0;      // output bytes
  bool fast = false;     // the message's own bytes, life version and header CRC rewritten
  int life = -1;         // fast: the life version to write, as the header's 16 bits (-1: keep the stored one)
  ambrycrc_put_desc d;   // general: the re-serialization
  ambrycrc::PropsFix fx;
};

// have_life: write life_version into the new header as given -- a batch's index value, negatives
// included (MessageInfo.LIFE_VERSION_FROM_FRONTEND is -1; ValidatingTransformer.java:90 writes
// msgInfo.getLifeVersion() unchanged, as the device batch does); otherwise keep the stored one.
uint32_t transform_plan(const uint8_t* region, uint64_t region_len, uint64_t off, bool have_life, int life_version,
                        int header_version, XPlan* x) {
  ambrycrc::MsgHeader H;
  uint64_t end = 0;
  const uint32_t st = off <= region_len ? verify(region + off, region_len - off, &H, &end) : (uint32_t)AMBRYCRC_MSG_BAD_LAYOUT;
  if (st) return st;
  const uint8_t* p = region + off;
  const int32_t bp = H.rel[1], upd = H.rel[2], um = H.rel[3], blob = H.rel[4];
  if (upd != -1 || bp == -1 || um == -1 || blob == -1) return AMBRYCRC_MSG_NOT_PUT;  // "cannot be anything rather than put record"
  // the deserializers' field reads (deserializeBlobEncryptionKey / Properties / UserMetadata / Blob,
  // MessageFormatRecord.java:1568-1833; msg_header.h put_fields); verify's record checks already hold for them
  const ambrycrc::PutFields f = ambrycrc::put_fields(p, H);
  // deserializeBlobProperties, re-serialized at VERSION_5 (record_fields.h; verify parsed it)
  const uint32_t stored = (uint32_t)f.props_len;
  ambrycrc::PropsFields pf;
  if (!f.ok || ambrycrc::props_parse<true>(p + bp + 2, stored, &pf) != 0) return AMBRYCRC_MSG_BAD_RECORD;
  if (!pf.ascii) return AMBRYCRC_MSG_NOT_ENCODABLE;
  x->fx = ambrycrc::props_fix_of(pf, stored);
  // A V3 message with a V3 blob record (isCompressed 0 or 1) and properties already canonical VERSION_5
  // bytes re-serializes at V3 to its own bytes but for the life version and the header CRC (the GPU fast path's rule,
  // region_proc.h transform_fast): one copy and the 32-byte header's CRC, instead of the layout,
  // copy and every record CRC again.
  if (header_version == 3 && H.version == 3 && f.blob_version == 3 && p[blob + 4] <= 1 && x->fx.version == 0) {
    x->fast = true;
    x->len = end;
    x->life = have_life && (uint16_t)life_version != (uint16_t)H.life ? (int)(uint16_t)life_version : -1;
    return 0;
  }
  x->d = ambrycrc::put_desc_of_stored(off, H, f, header_version, have_life ? life_version : H.life,
                                      ambrycrc::props_v5_len(x->fx));
  x->len = ambrycrc_put_layout(&x->d, nullptr);
  return x->len ? 0u : (uint32_t)AMBRYCRC_MSG_BAD_RECORD;
}

// Writes the planned message at out (x.len bytes of room).
int transform_emit(const uint8_t* region, uint64_t off, const XPlan& x, uint8_t* out) {
  if (x.fast) {
    memcpy(out, region + off, x.len);
    if (x.life >= 0) {
      ambrycrc::put_be16(out + 2, (uint32_t)x.life);
      ambrycrc::put_be64(out + 32, (uint64_t)ambrycrc_update(0, out, 32));
    }
    return AMBRYCRC_OK;
  }
  // the stored payload is copied (props_len bytes from props_src: the appendix's share of them comes
  // from the user-metadata record that follows, inside the message), then rewritten as V5 and its
  // record CRC recomputed
  const int rc = ambrycrc_serialize_put_host(&x.d, region, region, out, x.len, nullptr);
  if (rc) return rc;
  ambrycrc::PutLayout L;
  if (x.fx.version && ambrycrc::put_layout(x.d, L)) {
    ambrycrc::props_apply_fix(out + L.bp_rel + 2, x.fx);
    ambrycrc::put_seal_record(out, L, 2);
  }
  return AMBRYCRC_OK;
}

// Hard delete: the header's verdict and layout alone, then the user-metadata and blob spans (hard_delete.h).
uint32_t hd_header(const uint8_t* p, uint64_t rem, int* version, ambrycrc::HdSpans* s) {
  ambrycrc::MsgHeader H;
  ambrycrc::MsgLayout L;
  uint32_t st = decode(p, rem, &H);
  if (st == 0) st = ambrycrc::msg_layout(H, rem, &L);
  if (st) return st;
  *version = H.version;
  return ambrycrc::hd_header_spans(H, L, s);
}

}  // namespace

extern "C" {

int ambrycrc_hard_delete_message_cpu(uint8_t* region, uint64_t region_len, uint64_t off,
                                     const ambrycrc_hard_delete_info* recovery, int plan_only, uint32_t* status,
                                     ambrycrc_hard_delete_info* info) {
  if (!region || !status) return AMBRYCRC_EINVAL;
  if (info) memset(info, 0, sizeof *info);
  if (off > region_len) {
    *status = AMBRYCRC_MSG_BAD_LAYOUT;
    return AMBRYCRC_OK;
  }
  uint8_t* p = region + off;
  int hv = 0;
  ambrycrc::HdSpans s;
  uint32_t st = hd_header(p, region_len - off, &hv, &s);
  ambrycrc_hard_delete_info o;
  memset(&o, 0, sizeof o);
  if (st == 0 && recovery && recovery->header_version != 0) {  // "Skipping crc check": the records are not read
    if (ambrycrc::hd_recovery_ok(*recovery, s))
      o = ambrycrc::hd_info(hv, s, recovery->usermeta_size, recovery->blob_version, recovery->blob_type,
                            recovery->blob_size);
    else
      st = AMBRYCRC_MSG_BAD_RECORD;
  } else if (st == 0) {  // getUserMetadataInfo / getBlobRecordInfo: the two records' fields and CRCs
    const uint8_t* um = p + s.um_rel;
    const uint8_t* bl = p + s.blob_rel;
    st |= record_check(3, um, s.um_span);
    if ((uint64_t)ambrycrc_update(0, um, s.um_span - 8) != ld_be64(um + s.um_span - 8)) st |= AMBRYCRC_MSG_USERMETA_CRC;
    st |= record_check(4, bl, s.blob_span);
    if ((uint64_t)ambrycrc_update(0, bl, s.blob_span - 8) != ld_be64(bl + s.blob_span - 8)) st |= AMBRYCRC_MSG_BLOB_CRC;
    if (st == 0) {
      const int bv = (int)ld_be16(bl);
      o = ambrycrc::hd_info(hv, s, ld_be32(um + 2), bv, bv == 1 ? 0 : (int)ld_be16(bl + 2),
                            ld_be64(bl + ambrycrc::blob_head(bv) - 8));
    }
  }
  *status = st;
  if (st) return AMBRYCRC_OK;
  if (info) *info = o;
  if (plan_only) return AMBRYCRC_OK;
  // each record: prefix, zero body, CRC = the prefix CRC advanced over the zeros (never read back)
  uint8_t b[16];
  uint8_t* q = p + o.start;
  uint32_t n = ambrycrc::hd_um_prefix(o.usermeta_size, b);
  memcpy(q, b, n);
  memset(q + n, 0, o.usermeta_size);
  ambrycrc::put_be64(q + n + o.usermeta_size, (uint64_t)ambrycrc_zeros(ambrycrc_update(0, b, n), o.usermeta_size));
  q += s.um_span;
  n = ambrycrc::hd_blob_prefix(o.blob_version, o.blob_type, o.blob_size, b);
  memcpy(q, b, n);
  memset(q + n, 0, o.blob_size);
  ambrycrc::put_be64(q + n + o.blob_size, (uint64_t)ambrycrc_zeros(ambrycrc_update(0, b, n), o.blob_size));
  return AMBRYCRC_OK;
}

int ambrycrc_verify_message_cpu(const uint8_t* region, uint64_t region_len, uint64_t off, uint32_t* status,
                                uint64_t* msg_end) {
  if (!region || !status) return AMBRYCRC_EINVAL;
  ambrycrc::MsgHeader H;
  uint64_t end = 0;
  *status = off <= region_len ? verify(region + off, region_len - off, &H, &end) : (uint32_t)AMBRYCRC_MSG_BAD_LAYOUT;
  if (msg_end) *msg_end = end ? off + end : 0;
  return AMBRYCRC_OK;
}

// BlobStoreRecovery.recover (BlobStoreRecovery.java:43-139) as the plain sequential loop: the chain's
// acceptance test (recover.h), the verify above, the shared field reader (record_fields.h).
int ambrycrc_recover_messages_cpu(const uint8_t* region, uint64_t region_len, uint64_t start, size_t max_m,
                                  uint64_t* msg_off, ambrycrc_message_info* info, uint32_t* status,
                                  ambrycrc_recover_result* result) {
  if ((!region && region_len) || !msg_off || !result || start > region_len || max_m == 0 || max_m >= (1ull << 31))
    return AMBRYCRC_EINVAL;
  ambrycrc_recover_result r;
  memset(&r, 0, sizeof r);
  uint64_t off = start, first_bad = max_m;
  uint32_t bad_status = 0;
  while (off < region_len && r.chained < max_m) {
    uint64_t next = 0;
    const uint8_t* p = region + off;
    r.end_status = ambrycrc::msg_chain_accept(ambrycrc::HeaderBytes{p}, region_len - off, HostCrc{p}, &next);
    if (r.end_status) break;
    const size_t i = (size_t)r.chained++;
    msg_off[i] = off;
    ambrycrc::MsgHeader H;
    uint64_t end = 0;
    uint32_t st = verify(p, region_len - off, &H, &end);
    ambrycrc_message_info o;
    memset(&o, 0, sizeof o);
    if (st == 0) st = ambrycrc::message_info_fields(region + off, off, &o);
    if (info) info[i] = o;
    if (status) status[i] = st;
    if (st && first_bad == max_m) {
      first_bad = i;
      bad_status = st;
    }
    off += next;
  }
  for (size_t i = (size_t)r.chained; i < max_m; ++i) {
    msg_off[i] = ~0ull;
    if (info) memset(&info[i], 0, sizeof info[i]);
    if (status) status[i] = AMBRYCRC_MSG_BAD_LAYOUT;
  }
  r.recovered = r.chained;
  r.end_off = off;
  r.more = r.end_status == 0 && off != region_len ? 1u : 0u;
  if (first_bad != max_m) {
    r.recovered = first_bad;
    r.end_off = msg_off[first_bad];
    r.end_status = bad_status;
    r.more = 0;
  }
  *result = r;
  return AMBRYCRC_OK;
}

int ambrycrc_transform_message_cpu(const uint8_t* region, uint64_t region_len, uint64_t off, int life_version,
                                   int header_version, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                   uint32_t* status) {
  if (!region || !out_len || !status || header_version < 1 || header_version > 3 || life_version > 32767)
    return AMBRYCRC_EINVAL;
  *out_len = 0;
  XPlan x;
  *status = transform_plan(region, region_len, off, life_version >= 0, life_version, header_version, &x);
  if (*status) return AMBRYCRC_OK;
  if (!out || x.len > out_cap) {
    *status = AMBRYCRC_MSG_NO_ROOM;
    return AMBRYCRC_OK;
  }
  const int rc = transform_emit(region, off, x, out);
  if (rc) return rc;
  *out_len = x.len;
  return AMBRYCRC_OK;
}

// BlobIdTransformer.transform of one message (BlobIdTransformer.java:72-87,159-281; rekey.h): the
// semantics and status bits of ambrycrc_rekey_messages_dev. Every CRC of the output is hashed from the
// bytes written (the CLMUL loop), the blob record's in one pass with its copy's source still in cache.
int ambrycrc_rekey_message_cpu(const uint8_t* region, uint64_t region_len, uint64_t off,
                               const ambrycrc_rekey_desc* desc, const uint8_t* aux, uint64_t aux_len,
                               int life_version, int header_version, uint8_t* out, uint64_t out_cap,
                               uint64_t* out_len, uint32_t* status) {
  if (!region || !desc || !out_len || !status || (!aux && aux_len) || header_version < 1 || header_version > 3 ||
      life_version > 32767)
    return AMBRYCRC_EINVAL;
  *out_len = 0;
  *status = 0;
  const ambrycrc_rekey_desc& r = *desc;
  if (r.key_len == 0) return AMBRYCRC_OK;  // the converter had no key: skipped, not read
  if (!ambrycrc::rekey_desc_ok(r, aux_len)) {
    *status = AMBRYCRC_MSG_BAD_DESC;
    return AMBRYCRC_OK;
  }
  ambrycrc::MsgHeader H;
  uint64_t end = 0;
  *status = off <= region_len ? verify(region + off, region_len - off, &H, &end) : (uint32_t)AMBRYCRC_MSG_BAD_LAYOUT;
  if (*status) return AMBRYCRC_OK;
  ambrycrc_put_desc d;
  ambrycrc::RekeyFix x;
  *status = ambrycrc::rekey_plan(region, off, r, life_version >= 0, life_version, header_version, &d, &x);
  if (*status) return AMBRYCRC_OK;
  ambrycrc::PutLayout L;
  if (!ambrycrc::put_layout(d, L)) return AMBRYCRC_EINVAL;  // (rekey_plan checked it)
  if (!out || L.length > out_cap) {
    *status = AMBRYCRC_MSG_NO_ROOM;
    return AMBRYCRC_OK;
  }
  const bool repl = r.content_src != ambrycrc::kRekeyKeep;
  // bodies in place (the encryption-key and user-metadata records whole, their trailers verified), then the
  // header's, the properties' and the blob record's trailers hashed from the output
  ambrycrc::put_write_fixed(d, L, out);
  memcpy(out + L.hsize, aux + d.key_src, d.key_len);
  if (L.enc_rec) memcpy(out + L.enc_rel, region + d.enckey_src - 6, L.enc_rec);
  uint8_t* ps = out + L.bp_rel + 2;
  for (uint32_t j = 0; j < d.props_len; ++j)
    ps[j] = ambrycrc::rekey_props_byte(x, r, j, j < x.stored_len ? region[d.props_src + j] : 0);
  memcpy(out + L.um_rel, region + d.usermeta_src - 6, L.um_rec);
  if (d.blob_len) memcpy(out + L.blob_rel + 13, (repl ? aux : region) + d.blob_src, d.blob_len);
  for (uint32_t k = 0; k < ambrycrc::kPutSlots; k += 2) ambrycrc::put_seal_record(out, L, k);
  *out_len = L.length;
  return AMBRYCRC_OK;
}

// MessageFormatSend.fetchDataFromReadSet for one message (MessageFormatSend.java:112-242; send.h): the
// semantics, status and check bits of ambrycrc_send_messages_dev. ALL and BLOB run the whole verify
// (deserializeBlobAll); the metadata flags verify the header and hash only the records they read.
int ambrycrc_send_message_cpu(const uint8_t* region, uint64_t region_len, uint64_t off, uint64_t size, int flag,
                              uint8_t* out, uint64_t out_cap, ambrycrc_send_info* info, uint32_t* status) {
  if (!region || !info || !status || !ambrycrc::send_flag_ok(flag)) return AMBRYCRC_EINVAL;
  memset(info, 0, sizeof *info);
  info->out_off = ambrycrc::kSendNowhere;
  const bool in_region = off <= region_len;
  const uint64_t rem = in_region ? region_len - off : 0;
  const uint8_t* p = region + (in_region ? off : 0);
  const bool has_size = size != 0;
  const bool whole_verify = flag == AMBRYCRC_SEND_ALL || flag == AMBRYCRC_SEND_BLOB;
  ambrycrc::SendHeader H;
  memset(&H, 0, sizeof H);
  uint32_t hdr = AMBRYCRC_MSG_BAD_LAYOUT;
  if (in_region && !(has_size && size > rem)) {
    ambrycrc::MsgHeader D;
    hdr = decode(p, rem, &D);
    if (hdr == 0) hdr = ambrycrc::msg_layout(D, rem, &H);
  }
  // a record's CRC against its stored long
  auto crc_bad = [&](int k) {
    const uint8_t* q = p + H.rel[k];
    const uint64_t span = H.rend[k] - (uint64_t)H.rel[k];
    return (uint64_t)ambrycrc_update(0, q, span - 8) != ld_be64(q + span - 8);
  };
  const bool enc_bad = hdr == 0 && ambrycrc::send_reads_enckey(flag) && H.rel[0] != -1 && H.rel[2] == -1 && crc_bad(0);
  ambrycrc::SendPlan s;
  ambrycrc::send_plan(p, in_region, rem, has_size, size, flag, hdr, H, enc_bad, &s);
  *status = s.status;
  if (s.status) return AMBRYCRC_OK;
  uint32_t vbits = 0;  // the verify's bits that belong in check
  if (hdr == 0) {
    if (whole_verify) {
      ambrycrc::MsgHeader D;
      uint64_t end = 0;
      vbits = verify(p, rem, &D, &end);
    } else {
      for (int k = 1; k <= 3; k += 2)
        if (s.dst[k] != ambrycrc::kSendNone && crc_bad(k)) vbits |= kRecordBit[k];
    }
  }
  info->rel_off = s.rel_off;
  info->enckey_rel = s.enckey_rel;
  info->enckey_len = s.enckey_len;
  info->check = (vbits & ambrycrc::send_check_mask(flag)) | s.pre;
  if (!out || s.send_len > out_cap) {
    *status = AMBRYCRC_MSG_NO_ROOM;
    return AMBRYCRC_OK;
  }
  memcpy(out, p + s.rel_off, s.send_len);
  info->out_off = 0;
  info->send_len = s.send_len;
  return AMBRYCRC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- CPU batch forms
// The host entries' CPU leg (ambrycrc_set_host_policy; DESIGN.md §5 "host-resident dispatch"):
// ambrycrc_verify_messages_host / _transform_messages_host over messages in host memory, split
// across `threads` CPU threads by region bytes, each message through the single-message loops
// above. Same outputs as the device batch.
#include <algorithm>
#include <atomic>
#include <thread>
#include <memory>
#include <new>
#include <vector>

#include "ambrycrc_ctx.h"

namespace ambrycrc {
namespace detail {

namespace {
// fn(a, b) over contiguous index ranges of [0, m) holding about equal sums of weight(i).
template <class W, class F>
void split_run(size_t m, int threads, W weight, F fn) {
  threads = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), m));
  if (threads == 1) {
    fn((size_t)0, m);
    return;
  }
  std::vector<uint64_t> pre(m + 1, 0);
  for (size_t i = 0; i < m; ++i) pre[i + 1] = pre[i] + weight(i) + 64;  // + a per-message cost
  std::vector<size_t> cut(threads + 1, m);
  cut[0] = 0;
  for (int t = 1; t < threads; ++t)
    cut[t] = (size_t)(std::lower_bound(pre.begin(), pre.end(), pre[m] * (uint64_t)t / (uint64_t)threads) - pre.begin());
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) {
    if (cut[t] >= cut[t + 1]) continue;
    try {
      th.emplace_back(fn, cut[t], cut[t + 1]);
    } catch (...) {  // no thread (the C ABI does not throw): the part runs here
      fn(cut[t], cut[t + 1]);
    }
  }
  fn(cut[0], cut[1]);
  for (auto& x : th) x.join();
}

uint64_t extent_of(const uint8_t* region, uint64_t region_len, uint64_t off) {
  return off >= region_len ? 0 : message_extent_of(region + off, region_len - off);
}
}  // namespace

int verify_messages_cpu(const uint8_t* region, uint64_t region_len, const uint64_t* msg_off, size_t m,
                        uint32_t* status, uint64_t* msg_end, int threads) {
  std::atomic<int> rc{AMBRYCRC_OK};  // written by any worker
  split_run(m, threads, [&](size_t i) { return extent_of(region, region_len, msg_off[i]); },
            [&](size_t a, size_t b) {
              for (size_t i = a; i < b; ++i) {
                uint64_t e = 0;
                if (ambrycrc_verify_message_cpu(region, region_len, msg_off[i], &status[i], &e) != AMBRYCRC_OK)
                  rc.store(AMBRYCRC_EINVAL);
                if (msg_end) msg_end[i] = e;
              }
            });
  return rc.load();
}

int transform_messages_cpu(const uint8_t* region, uint64_t region_len, const uint64_t* msg_off, size_t m,
                           const int16_t* life_version, int header_version, uint8_t* out, uint64_t out_cap,
                           uint64_t* out_off, uint64_t* out_len, uint32_t* status, int threads) {
  // every message planned in parallel (verified, its output length known), placed in message order
  // as the device batch packs it (NO_ROOM once the running sum passes out_cap), then emitted in
  // parallel straight into `out` (round 5's first form transformed into a scratch copy of the region
  // and packed it after: two more passes over the bytes and a fresh allocation's page faults)
  std::vector<XPlan> plan(m);
  split_run(m, threads, [&](size_t i) { return extent_of(region, region_len, msg_off[i]); }, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; ++i)
      status[i] = transform_plan(region, region_len, msg_off[i], life_version != nullptr,
                                 life_version ? life_version[i] : 0, header_version, &plan[i]);
  });
  std::vector<uint64_t> pos(m, ~0ull);  // output position, ~0: not placed
  uint64_t vpos = 0;
  for (size_t i = 0; i < m; ++i) {
    if (status[i] == 0 && plan[i].len) {
      if (vpos + plan[i].len <= out_cap)
        pos[i] = vpos;
      else
        status[i] = AMBRYCRC_MSG_NO_ROOM;
      vpos += plan[i].len;
    }
    if (out_off) out_off[i] = pos[i];
    out_len[i] = pos[i] == ~0ull ? 0 : plan[i].len;
  }
  std::atomic<int> rc{AMBRYCRC_OK};  // written by any worker
  split_run(m, threads, [&](size_t i) { return pos[i] == ~0ull ? 0 : plan[i].len; }, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; ++i)
      if (pos[i] != ~0ull && transform_emit(region, msg_off[i], plan[i], out + pos[i]) != AMBRYCRC_OK)
        rc.store(AMBRYCRC_EINVAL);
  });
  return rc.load();
}

}  // namespace detail
}  // namespace ambrycrc
