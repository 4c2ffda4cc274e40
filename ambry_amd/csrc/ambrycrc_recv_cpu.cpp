// ambrycrc_recv_cpu.cpp -- one payload of a GetResponse body on the CPU (ambrycrc_receive_blob_cpu):
// recv.h's whole receive with the CLMUL host loop (ambrycrc_update) for the CRCs. The semantics and status
// bits are ambrycrc_receive_blobs_dev's.
#include "../../include/ambrycrc.h"

#include "recv.h"

extern "C" {

int ambrycrc_receive_blob_cpu(const uint8_t* payload, uint64_t avail, int flag, uint64_t lo, uint64_t hi, uint8_t* out,
                              uint64_t out_cap, ambrycrc_recv_info* info, uint32_t* status) {
  if ((!payload && avail) || !info || !status || !ambrycrc::recv_flag_ok(flag)) return AMBRYCRC_EINVAL;
  const auto crc = [](const uint8_t* p, uint64_t n) { return ambrycrc_update(0, p, (size_t)n); };
  ambrycrc::recv_blob_host(payload, avail, flag, lo, hi, out, out_cap, crc, info, status);
  return AMBRYCRC_OK;
}

}  // extern "C"
