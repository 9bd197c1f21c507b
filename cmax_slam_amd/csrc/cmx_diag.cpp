// cmx_diag.cpp -- read-only diagnostic read-backs (include/cmax_hip_diag.h).  Nothing here queues a kernel or changes what a
// context holds: the tests read what the evaluation paths left behind.
#include "cmx_recon_state.hpp"

// Jt as the last adjoint image pass left it.  No evaluation path keeps a record of which tiles that pass wrote: the caller derives
// the set from the forward plane (tests/dense_image_ops.py: compare_set).
int cmx_diag_get_adjoint_plane(cmx_ctx *c, int which, float *host) {
  if (!c || !host) return fail(c, CMX_ERR_INVALID_ARG, "null context / host buffer");
  if (c->group) return fail(c, CMX_ERR_INVALID_ARG, "the adjoint plane of a group lives in its members: not available on a group handle");
  if (which != CMX_DIAG_JT_EVAL && which != CMX_DIAG_JT_RECON) return fail(c, CMX_ERR_INVALID_ARG, "adjoint plane %d does not exist", which);
  const float *src = nullptr;
  size_t np = 0;
  if (which == CMX_DIAG_JT_EVAL) {
    np = (size_t)c->imgW * c->imgH;
    if (c->d_itilde && np > 0 && c->itilde_cap >= np) src = c->d_itilde;
  } else if (c->kind == KIND_BE && c->recon) {
    np = (size_t)c->Wp * c->Hp;
    src = c->recon->d_jt;
  }
  if (!src) return fail(c, CMX_ERR_STATE, "no adjoint image pass has run: the plane was never allocated");
  int rc = bind_device(c);
  if (rc) return rc;
  if (c->stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(host, src, np * sizeof(float), hipMemcpyDeviceToHost));
  return CMX_OK;
}

// The front end's forward plane: plane 0 of the buffer the last fe_accumulate voted into, whichever call ran it.
int cmx_diag_get_forward_plane(cmx_ctx *c, float *host) {
  if (!c || !host) return fail(c, CMX_ERR_INVALID_ARG, "null context / host buffer");
  if (c->group) return fail(c, CMX_ERR_INVALID_ARG, "the forward plane of a group lives in its members: not available on a group handle");
  if (c->kind != KIND_FE) return fail(c, CMX_ERR_STATE, "not a front-end context");
  const size_t np = (size_t)c->W * c->H;
  if (!c->have_data || !c->accumulated || !c->d_accum || np == 0 || c->accum_count < np)
    return fail(c, CMX_ERR_STATE, "no accumulate since the packet was set: the plane holds no evaluation's votes");
  int rc = bind_device(c);
  if (rc) return rc;
  if (c->stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(host, c->d_accum, np * sizeof(float), hipMemcpyDeviceToHost));
  return CMX_OK;
}
