/* givepose_wpack.h -- the weight-pack family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * One-time permutations of packed fp16 weights into the order a kernel's DMA wants, on the device: fp16 in, fp16 out, no host round trip.
 * The weights are constant between forwards, so a pack runs where the weights are packed (PoseNet._pack) and never per forward; the
 * after-step repack (givepose_repack.h) writes the same layouts as views of the fp32 parameters.
 *
 * The family has its own header and prefix (gpw_) like givepose_repack.h (gpr_), whose conventions apply: device pointers to caller-owned
 * buffers, no allocation, no synchronisation, a hipStream_t `stream`, 0 or a negative gp_status, gp_last_error().
 */
#ifndef GIVEPOSE_WPACK_H
#define GIVEPOSE_WPACK_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 3x3 conv weights w[n][kh*3 + kw][Cin] (gp_gemm's conv layout, K = tap * Cin + ci) -> the chunk-major copy
 * wcm[n][ci / 32][kh*3 + kw][ci % 32] that gp_gemm_desc.W_cm takes: the window conv walks K channel chunk outer / tap inner, and in this
 * order two consecutive steps of that walk are one 128-byte line of a row.  A pure permutation inside every row of 9 Cin values.
 * N rows, Cin % 32 == 0, both pointers 16-byte aligned, w != wcm. */
int gpw_conv3_pack_wcm(const void* w, void* wcm, int N, int Cin, void* stream);

/* sizeof(gp_gemm_desc) of the header the library was built from.  gp_gemm_desc.W_cm was appended without a new GP_ABI_VERSION, so a
 * binding checks this number against its own struct before it hands a descriptor to gp_gemm (givepose_amd._lib.load does). */
int gpw_gemm_desc_bytes(void);

#ifdef __cplusplus
}
#endif
#endif
