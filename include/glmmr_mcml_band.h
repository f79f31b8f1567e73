/*
 * glmmr_mcml_band.h -- test hooks of the row-tile extents of the banded HMC products of libglmmr_mcml_hip.so (csrc/band_plan.h,
 * csrc/dgemm_band.h): part of the C ABI, included by glmmr_mcml_c.h (include that header; this one relies on its types and error
 * codes).  For tests/ only.
 */
#ifndef GLMMR_MCML_BAND_H
#define GLMMR_MCML_BAND_H
#ifndef GLMMR_MCML_C_H
#error "include glmmr_mcml_c.h, which includes this header"
#endif

/* The extents: per 80-row band of a banded product's A operand and per 16-row tile of the band, the first and the one-past-last
 * K substep (4 columns) that holds a nonzero, 10 ints per band; a row tile without a nonzero, or past the last row: two equal
 * values.  Inside a band's K-tile range the kernel issues the MFMAs of a row tile only between them
 * (GLMMR_MCML_BAND_ROWTILES=0, read per launch: every MFMA of the K tiles, as before the extents). */

/* read-only: the host copy of the extents of the sampler's forward (which = 0) or backward (which = 1) operand, as many ints as
 * fit `cap` of ext (nullable with cap = 0); out3 = [bands, MFMAs per 16-column strip inside the extents, MFMAs per strip of the
 * whole K tiles].  Zeros while the sparse operator is active. */
int glmmr_mcml_dbg_band_extents(glmmr_mcml_ctx* ctx, int which, int* ext, int cap, long long* out3);
/* C = A B through the banded kernel as glmmr_mcml_dbg_dgemm_band_form runs it (form 0: eight waves that each load and multiply,
 * 1: four MFMA waves fed by four DMA waves), and the host copy of the operand's extents into ext_out (ext_cap ints of room, at
 * least 10 per band); mfmas_issued = MFMAs per 16-column strip the launch issued (the switch honoured) */
int glmmr_mcml_dbg_dgemm_band_ext(int M, int N, int K, const double* A, int lda, const double* B, int ldb, double* C,
                                  int ldc, int form, int* ext_out, int ext_cap, long long* mfmas_issued);

#endif
