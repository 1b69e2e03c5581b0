/* givepose_repack.h -- the weight-repack family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * What PoseNet._pack does on the host after every optimiser step -- permute, concatenate, fold and round the reference-layout fp32
 * parameters into the tensors the forward's kernels read -- as a fixed number of launches on the device, in place: every packed
 * tensor keeps its address, so the forward's plans and captured hipGraphs stay valid.  A repack is at most GPR_REPACK_LAUNCHES
 * launches whatever the number of tensors or layers.
 *
 * The family has its own header and prefix (gpr_) next to givepose_optim.h (gpo_), whose conventions apply: device pointers to
 * caller-owned buffers, no allocation on the device, no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative
 * gp_status, gp_last_error(), a size query that answers 0 for what the entry point refuses.
 *
 * Tables.  The caller describes the repack ONCE per model with four HOST arrays (the pointers inside them are device pointers):
 *   gpr_entry    one strided view of an fp32 source, up to 4-D, written densely (row-major over the view's dims) at an element offset
 *                of a destination, as fp32, as fp16 (round to nearest even), or as the hi / lo' fp16 planes of the split-operand mode
 *                (hi = fp16(v), lo' = fp16((v - hi) 2^GP_SPLIT_SHIFT): gp_split_planes' arithmetic);
 *   gpr_bnfold   eval BatchNorm1d folded into the 1x1 conv in front of it (fp32, the host's expression, every operation correctly rounded);
 *   gpr_matfold  out = A B (+ add), accumulated in fp64 in k order and rounded once; an entry of level 1 may read the fp64 result of
 *                an entry of level 0.
 * gpr_tables_upload checks them -- every view and every fold against the element counts the caller states for its tensors, so that no
 * kernel can read or write outside what the tables declare --, cuts every entry into chunks of at most GPR_CHUNK destination elements
 * (a workgroup's entry, first element and count) and sends all tables to `tables` with ONE asynchronous copy from the caller's `stage`.  gpr_repack reads them there; per call nothing is
 * built, copied or sent.  The fold results are written to fp32 scratch that entries name as their source.
 *
 * Launches of gpr_repack, in stream order: (1) the BatchNorm folds, (2) the matrix folds of level 0, (3) those of level 1, (4) the
 * copy over all chunks.  A launch whose table is empty is skipped: the fp16 mode has all four (enc0.xyz_m is the one level-1 fold),
 * the fp32 and split-operand modes three (GPR_REPACK_LAUNCHES_F32).  fc2_wp, the fused MLP's column order of fc2 (in every block
 * of 32 hidden units k-slot fq 8 + nt 4 + j takes unit nt 16 + fq 4 + j: gp_convnext_mlp_pack_w2), is a 4-D view of fc2.weight and
 * so an entry of the copy like any other: no launch per block, no fp16 surcharge.
 *
 * The copy.  Element i of a chunk belongs to thread (i / 8) % 256 where the entry's view is one contiguous run, and eight elements
 * move as two 16-byte loads and one or two 16-byte stores where source and destination are 16-byte aligned, else one by one; any
 * other view is gathered one element per thread (destination-contiguous, so the stores coalesce).  Every element is computed
 * from its own source value alone, so the bits depend neither on alignment nor on the chunking.  No atomics.
 */
#ifndef GIVEPOSE_REPACK_H
#define GIVEPOSE_REPACK_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPR_CHUNK 4096               /* destination elements per workgroup: 16 per lane */
#define GPR_REPACK_LAUNCHES 4        /* BatchNorm folds, matrix folds level 0, level 1, copy (fp16 mode) */
#define GPR_REPACK_LAUNCHES_F32 3    /* fp32 and split-operand modes: no level-1 fold */
#define GPR_MAX_ENTRIES 65536
#define GPR_MAX_DIMS 4
#define GPR_KIND_F32 0
#define GPR_KIND_F16 1
#define GPR_KIND_SPLIT 2

typedef struct gpr_entry {
    const float* src;                /* fp32 source: a parameter, a buffer or fold scratch */
    void* dst;                       /* destination tensor: fp32 (F32), fp16 (F16) or plane 0 of the fp16 planes (SPLIT) */
    long long src_numel, dst_numel;  /* elements of the source and of the destination (of ONE plane for SPLIT): the bounds */
    long long src_off;               /* first element of the view */
    long long dst_off;               /* element of the destination (of each plane) the view's first element goes to */
    long long plane_stride;          /* SPLIT: halfs from plane 0 to plane 1 (>= dst_numel), else 0 */
    long long strides[GPR_MAX_DIMS]; /* source strides in elements, outermost first; >= 0 */
    int dims[GPR_MAX_DIMS];          /* the view, outermost first; unused leading dims are 1 */
    int kind;                        /* GPR_KIND_* */
    int pad;
} gpr_entry;

typedef struct gpr_bnfold {          /* sc = bn_w / sqrt(var + eps);  w_out[c][k] = w[c][k] sc[c];  b_out[c] = (b[c] - mean[c]) sc[c] + bn_b[c] */
    const float *w, *b, *bn_w, *bn_b, *mean, *var;
    float *w_out, *b_out;
    long long w_numel, c_numel;      /* elements of w and of w_out (>= C K); of each of the six per-channel arrays (>= C): the bounds */
    int C, K;
    float eps;
    int pad;
} gpr_bnfold;

typedef struct gpr_matfold {         /* out[m][n] = sum_k A[m a_rs + k] B[k b_rs + n] (+ add[m]), fp64, k ascending, rounded once */
    const float* A;
    const void* B;                   /* fp32, or fp64 where b_f64 (the out64 of a level-0 entry) */
    const float* add;                /* may be null */
    float* out32;                    /* out32[m ld32 + n]; may be null if out64 is given */
    double* out64;                   /* out64[m ld64 + n], unrounded; may be null */
    long long a_numel, b_numel, add_numel, out32_numel, out64_numel;   /* elements that lie behind each pointer: the bounds */
    int M, N, K;
    int a_rs, b_rs, ld32, ld64;
    int b_f64, level, pad;
} gpr_matfold;

typedef struct gpr_info {            /* filled by gpr_tables_upload, handed back to gpr_repack unchanged */
    long long bytes;
    long long off_chunks, off_bn, off_mat, off_mchunks;
    int n_entries, n_chunks, n_bn, n_bn_blocks, n_mat, n_mchunks0, n_mchunks1, pad;
} gpr_info;

/* Bytes of the device tables for these host tables; 0 for what gpr_tables_upload would refuse. */
long long gpr_tables_bytes(const gpr_entry* entries, int n, const gpr_bnfold* bn, int n_bn, const gpr_matfold* mat, int n_mat);
/* Checks the host tables, lays them out in `stage` (HOST memory of the caller, tables_bytes long, ideally pinned) and sends them from there
 * to `tables` (device, 256-byte aligned, tables_bytes >= gpr_tables_bytes) with one asynchronous copy.  The caller keeps `stage` alive and
 * unchanged until that copy has run on `stream`; the library keeps no staging buffer of its own. */
int gpr_tables_upload(const gpr_entry* entries, int n, const gpr_bnfold* bn, int n_bn, const gpr_matfold* mat, int n_mat, void* stage,
                      void* tables, long long tables_bytes, gpr_info* info, void* stream);
/* One repack: the launches above on `stream`, in place. */
int gpr_repack(const void* tables, const gpr_info* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
