// gpx_sparse.inc — the inducing-point GP's entry points (include/gpx.h: gpx_sparse_*; DESIGN.md §3.4r), included at the end
// of gpx_api.hip inside its extern "C" block.  fp64, one device.  Its kernels are in gpx_sparse.hip; the factorisations, the
// whitening solve and the kernel builds are the dense engine's (chol_enqueue, solve_fwd_enqueue, launch_kbuild_*).
//
// The order of the fit is part of the model's definition: the cross-kernel rows of a chunk are whitened by L^-1 (a right
// solve of the chunk against L^T, as gpx_predict's variance stage) BEFORE they are contracted over the observations.
// Forming K_uf S^-1 K_fu first and whitening the m x m result halves the work and loses the result (DESIGN.md).

extern "C++" {
namespace {

constexpr int SP_NB = 1024;         // panel width of both factorisations and block width of the solves
constexpr int SP_MAX_K = 8;         // target columns
constexpr int64_t SP_CHUNK_MAX = 65536;

// Rows per chunk when the caller leaves the choice to the library: a function of m ONLY (the split of the contraction, and
// with it the bits of the result, follow from (m, chunk)) — about 2^25 elements of bordered rows, 1024 ... 65536 rows.
int64_t sparse_auto_chunk(int64_t mpad) {
  const int64_t c = ((int64_t)1 << 25) / (mpad + RHS_ROWS) / TILE * TILE;
  return std::max<int64_t>(1024, std::min(SP_CHUNK_MAX, c));
}

int sparse_handle_refused(gpx_handle* h, const char* fn) {
  if (h->group || h->in_group) return fail(h, GPX_E_UNSUPPORTED, fn, "device groups are not supported (single-device GPX_F64 handles only)");
  if (h->cfg.world > 1 || h->comm) return fail(h, GPX_E_UNSUPPORTED, fn, "shards are not supported (single-device GPX_F64 handles only)");
  if (h->cfg.dtype != GPX_F64) return fail(h, GPX_E_UNSUPPORTED, fn, "GPX_F32 / GPX_MIXED handles are not supported (GPX_F64 only)");
  return GPX_OK;
}

// a sparse entry point on a handle without a sparse fit
int sparse_unfitted(gpx_handle* h, const char* fn) {
  if (h->sp.fitted) return GPX_OK;
  return fail(h, GPX_E_ARG, fn,
              h->fitted ? "the handle holds a dense fit, not an inducing-point fit: gpx_sparse_* serves gpx_sparse_fit only (use "
                          "gpx_predict and its family)"
                        : "handle has no successful gpx_sparse_fit");
}

InvWork<double> sparse_inv_work(gpx_handle* h) {
  InvWork<double> iw;
  iw.W = (double*)h->sp.Wblk.p;
  iw.U = (double*)h->sp.Ublk.p;
  iw.ldu = SP_NB + LD_SKEW;
  iw.nbw = SP_NB;
  iw.aux = h->st3;
  return iw;
}

int sparse_fit_impl(gpx_handle* h, const void* X, const void* y, const void* w, int64_t N, int32_t d, int32_t k, const void* Z,
                    int64_t m, const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter, int64_t chunk,
                    int32_t mem_kind, double sum_log_s2, double sum_inv_s2, int64_t* info, bool retried = false) {
  gpx_handle::Sparse& sp = h->sp;
  const int64_t mpad = round_up(m, TILE), nb_ = mpad + RHS_ROWS;  // nb_: columns of a bordered chunk row = edge of B
  const int64_t ld = nb_ + LD_SKEW, ldp = SP_NB + LD_SKEW;
  const int64_t C = chunk > 0 ? round_up(chunk, TILE) : sparse_auto_chunk(mpad);
  const int64_t cb = std::min(C, round_up(N, TILE));  // rows the chunk buffers hold
  const int64_t nblk = (mpad + SP_NB - 1) / SP_NB;
  int rc;
  {  // what the fit allocates, against what is free plus what the handle's buffers of the same names hold already
    const double need = 8.0 * (2.0 * nb_ * ld + 2.0 * nb_ * ldp + (double)nblk * SP_NB * SP_NB + (double)SP_NB * ldp +
                               (double)cb * ld + (double)syrk_tn_part_elems(nb_, C) + (double)cb * (2 * d + k + 1) +
                               2.0 * mpad * d + 2.0 * (mpad / KB) * KB * KB) + 8192;
    const double have = (double)sp.L.cap + sp.B.cap + sp.P.cap + sp.Wblk.cap + sp.Ublk.cap + sp.Kc.cap + sp.part.cap + sp.Xc.cap +
                        sp.Xsc.cap + sp.Yc.cap + sp.Wc.cap + sp.Z.cap + sp.Zs.cap + sp.WinvL.cap + sp.WinvB.cap;
    size_t freeb = 0, totalb = 0;
    HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
    if (need > (double)freeb + have) {
      char buf[256];
      snprintf(buf, sizeof buf, "gpx_sparse_fit: m = %lld inducing points with chunks of %lld rows need %.3f GB of device memory, "
               "%.3f GB are free", (long long)m, (long long)cb, need / 1e9, ((double)freeb + have) / 1e9);
      return fail(h, GPX_E_NOMEM, buf);
    }
  }
  sp.fitted = false;
  sp.N = N, sp.m = m, sp.mpad = mpad, sp.chunk = C, sp.ld = ld, sp.sum_inv_s2 = sum_inv_s2;
  h->N = N, h->d = d, h->k = k, h->n_ls = n_ls, h->sf2 = sf2, h->sn2 = sn2, h->jitter = jitter;
  gpx_timings& tm = h->tm;
  tm.h2d = tm.kbuild = tm.chol = tm.solve = tm.logdet = tm.fit_total = 0;
  tm.chol_diag = tm.chol_trsm = tm.chol_strip = tm.chol_syrk = tm.syrk_flops = tm.comm = 0;
  tm.syrk_launches = 0;
  tm.kbuild_bytes = 8.0 * ((double)N * (mpad + d) + (double)m * (m + 1) / 2.0);

  if ((rc = flag_handover_probe(h))) return rc;
  if ((rc = ensure(h, h->ls, MAX_D * 8))) return rc;
  if ((rc = ensure(h, sp.Z, (size_t)m * d * 8)) || (rc = ensure(h, sp.Zs, (size_t)mpad * d * 8))) return rc;
  if ((rc = ensure(h, sp.L, (size_t)nb_ * ld * 8)) || (rc = ensure(h, sp.B, (size_t)nb_ * ld * 8))) return rc;
  if ((rc = ensure(h, sp.WinvL, (size_t)(mpad / KB) * KB * KB * 8)) || (rc = ensure(h, sp.WinvB, (size_t)(mpad / KB) * KB * KB * 8)))
    return rc;
  if ((rc = ensure(h, sp.P, (size_t)2 * nb_ * ldp * 8))) return rc;
  if ((rc = ensure(h, sp.Wblk, (size_t)nblk * SP_NB * SP_NB * 8)) || (rc = ensure(h, sp.Ublk, (size_t)SP_NB * ldp * 8))) return rc;
  if ((rc = ensure(h, sp.info, 128)) || (rc = ensure(h, sp.scal, 64 * 8))) return rc;
  if ((rc = ensure(h, sp.Xc, (size_t)cb * d * 8)) || (rc = ensure(h, sp.Xsc, (size_t)cb * d * 8))) return rc;
  if ((rc = ensure(h, sp.Yc, (size_t)cb * k * 8)) || (w && (rc = ensure(h, sp.Wc, (size_t)cb * 8)))) return rc;
  if ((rc = ensure(h, sp.Kc, (size_t)cb * ld * 8))) return rc;
  if ((rc = ensure(h, sp.part, (size_t)syrk_tn_part_elems(nb_, C) * 8))) return rc;

  double* dL = (double*)sp.L.p;
  double* dB = (double*)sp.B.p;
  double* dKc = (double*)sp.Kc.p;
  double* dP = (double*)sp.P.p;
  double* dScal = (double*)sp.scal.p;  // [0] tr(A A^T), [1 + c] |yt_c|^2, [16] log|B|, [17 + c] |c_c|^2
  int* dInfoL = (int*)sp.info.p;       // two 64-byte info blocks (chol_enqueue's layout): Kuu, B
  int* dInfoB = dInfoL + 16;
  const double* dZs = (const double*)sp.Zs.p;
  const double* dls = (const double*)h->ls.p;
  const int kernel = h->cfg.kernel;
  {
    PhaseScope total(h, &tm.fit_total);
    {
      PhaseScope ps(h, &tm.h2d);
      if ((rc = copy_in(h, sp.Z.p, Z, (size_t)m * d * 8, mem_kind))) return rc;
      if ((rc = copy_in(h, h->ls.p, lengthscale, (size_t)n_ls * 8, GPX_MEM_HOST))) return rc;
      HIPCHK(h, hipMemsetAsync(sp.info.p, 0, 128, h->st));
      HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)dInfoL, INT_MAX, 1, h->st));
      HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)dInfoB, INT_MAX, 1, h->st));
      HIPCHK(h, hipMemsetAsync(sp.scal.p, 0, 64 * 8, h->st));
    }
    {  // Kuu = sf2 k(Z, Z) + jitter I (padded rows: identity)
      PhaseScope ps(h, &tm.kbuild);
      launch_scale_points<double>((const double*)sp.Z.p, m, mpad, d, dls, n_ls, (double*)sp.Zs.p, h->st);
      HIPCHK(h, hipMemsetAsync(dL, 0, (size_t)nb_ * ld * 8, h->st));
      launch_kbuild_sym<double>(kernel, dZs, m, mpad, d, sf2, jitter, dL, ld, h->st);
    }
    {
      PhaseScope ps(h, &tm.chol);
      InvWork<double> iw = sparse_inv_work(h);
      if ((rc = chol_enqueue<double>(h, dL, ld, mpad, SP_NB, (double*)sp.WinvL.p, dP, dP + nb_ * ldp, ldp, dInfoL, 0, false, 0, &iw)))
        return rc;
      HIPCHK(h, hipMemsetAsync(dB, 0, (size_t)nb_ * ld * 8, h->st));
    }
    for (int64_t c0 = 0; c0 < N; c0 += C) {  // the chunks, in order: build, whiten, contract
      const int64_t rows = std::min(C, N - c0), rp = round_up(rows, TILE);
      {
        PhaseScope ps(h, &tm.kbuild);
        if ((rc = copy_in(h, sp.Xc.p, (const double*)X + c0 * d, (size_t)rows * d * 8, mem_kind))) return rc;
        if ((rc = copy_in(h, sp.Yc.p, (const double*)y + c0 * k, (size_t)rows * k * 8, mem_kind))) return rc;
        if (w && (rc = copy_in(h, sp.Wc.p, (const double*)w + c0, (size_t)rows * 8, mem_kind))) return rc;
        launch_scale_points<double>((const double*)sp.Xc.p, rows, rp, d, dls, n_ls, (double*)sp.Xsc.p, h->st);
        launch_kbuild_cross<double>(kernel, (const double*)sp.Xsc.p, rows, rp, dZs, m, mpad, d, sf2, dKc, ld, h->st);
        launch_sparse_border(dKc, ld, rows, rp, mpad, (const double*)sp.Yc.p, k, w ? (const double*)sp.Wc.p : nullptr, sn2, h->st);
      }
      {
        PhaseScope ps(h, &tm.solve);
        if ((rc = solve_fwd_enqueue<double>(h, dKc, rp, dL, ld, mpad, SP_NB, (const double*)sp.WinvL.p))) return rc;
        launch_syrk_tn(dB, ld, nb_, dKc, ld, rows, C, (double*)sp.part.p, 1, h->st);
      }
    }
    {  // B = I + A A^T with b^T = (A yt)^T below it; its factorisation leaves c^T = (LB^-1 b)^T there
      PhaseScope ps(h, &tm.chol);
      launch_sparse_close(dB, ld, mpad, k, dScal, h->st);
      InvWork<double> iw = sparse_inv_work(h);
      if ((rc = chol_enqueue<double>(h, dB, ld, mpad, SP_NB, (double*)sp.WinvB.p, dP, dP + nb_ * ldp, ldp, dInfoB, 0, false, RHS_ROWS,
                                     &iw)))
        return rc;
    }
    {
      PhaseScope ps(h, &tm.logdet);
      launch_logdet<double>(dB, ld, mpad, dScal + 16, h->st);
      for (int c = 0; c < k; ++c) launch_rows_sumsq(dB + (mpad + c) * ld, ld, 1, mpad, dScal + 17 + c, h->st);
    }
  }
  int hinfo[2] = {0, 0};
  double scal[32];
  HIPCHK(h, hipMemcpyAsync(&hinfo[0], dInfoL, sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(&hinfo[1], dInfoB, sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(scal, dScal, sizeof scal, hipMemcpyDeviceToHost, h->st));
  if ((rc = finish_call(h))) return rc;
  if (hinfo[0] < 0 || hinfo[1] < 0) {  // a parked stream timed out: once more with hipEvents (fit_impl does the same)
    if (retry_with_events(h, retried))
      return sparse_fit_impl(h, X, y, w, N, d, k, Z, m, lengthscale, n_ls, sf2, sn2, jitter, chunk, mem_kind, sum_log_s2, sum_inv_s2,
                             info, true);
    return fail(h, GPX_E_HIP, "gpx_sparse_fit: a stream parked on a device flag timed out (set GPX_CHAIN_FLAG=0)");
  }
  tm.handover_flags = chain_flag_enabled(h) ? 1.0 : 0.0;
  tm.handover_retries = (double)h->flag_retries;
  *info = hinfo[0] != INT_MAX ? (int64_t)hinfo[0] : hinfo[1] != INT_MAX ? m + (int64_t)hinfo[1] : 0;
  if (*info == 0) {
    bool finite = std::isfinite(scal[0]) && std::isfinite(scal[16]);
    for (int c = 0; c < k; ++c) {
      sp.elbo[c] = -0.5 * (double)N * std::log(2.0 * M_PI) - 0.5 * scal[16] - 0.5 * sum_log_s2 - 0.5 * scal[1 + c] +
                   0.5 * scal[17 + c] - 0.5 * sf2 * sum_inv_s2 + 0.5 * scal[0];
      finite = finite && std::isfinite(sp.elbo[c]);
    }
    if (!finite) *info = m + 1;  // (values that are not finite passed both factorisations: never a fit with NaN results)
  }
  sp.fitted = (*info == 0);
  return GPX_OK;
}

// T1^T = K* L^-T in V1 and T2^T = T1^T LB^-T in V2 for `mp` padded rows (mv valid) of scaled query points Qs
int sparse_whiten_queries(gpx_handle* h, const double* Qs, int64_t mv, int64_t mp, double* V1, double* V2) {
  gpx_handle::Sparse& sp = h->sp;
  int rc;
  {
    PhaseScope ps(h, &h->tm.kstar);
    launch_kbuild_cross<double>(h->cfg.kernel, Qs, mv, mp, (const double*)sp.Zs.p, sp.m, sp.mpad, h->d, h->sf2, V1, sp.ld, h->st);
  }
  PhaseScope ps(h, &h->tm.trsm);
  if ((rc = solve_fwd_enqueue<double>(h, V1, mp, (const double*)sp.L.p, sp.ld, sp.mpad, SP_NB, (const double*)sp.WinvL.p))) return rc;
  launch_copy2d<double>(V2, sp.ld, V1, sp.ld, mp, sp.mpad, h->st);
  return solve_fwd_enqueue<double>(h, V2, mp, (const double*)sp.B.p, sp.ld, sp.mpad, SP_NB, (const double*)sp.WinvB.p);
}

// mean^T columns [m0, m0 + mp) of MT = c^T T2
void sparse_mean_product(gpx_handle* h, double* MT, int64_t ldm, const double* V2, int64_t mp) {
  gpx_handle::Sparse& sp = h->sp;
  PhaseScope ps(h, &h->tm.mean);
  launch_gemm_nt<double>(64, MT, ldm, (const double*)sp.B.p + sp.mpad * sp.ld, sp.ld, V2, sp.ld, RHS_ROWS, mp, sp.mpad, 0, 1, h->st);
}

int sparse_predict_impl(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, int32_t mem_kind) {
  gpx_handle::Sparse& sp = h->sp;
  const int64_t Mpad = round_up(M, TILE), ldm = Mpad + LD_SKEW, ld = sp.ld;
  const int64_t MB = std::min<int64_t>(h->env.pred_batch, Mpad);
  const int k = h->k;
  reset_predict_clocks(h->tm);
  int rc;
  if ((rc = ensure_queries<double>(h, M))) return rc;
  if ((rc = ensure(h, h->scr.SV1, (size_t)MB * ld * 8)) || (rc = ensure(h, h->scr.SV2, (size_t)MB * ld * 8))) return rc;
  if ((rc = ensure(h, h->scr.MT, (size_t)RHS_ROWS * ldm * 8))) return rc;
  if ((rc = ensure(h, h->meanout, (size_t)M * k * 8)) || (rc = ensure(h, h->var, (size_t)Mpad * 8))) return rc;
  double* V1 = (double*)h->scr.SV1.p;
  double* V2 = (double*)h->scr.SV2.p;
  {
    PhaseScope total(h, &h->tm.predict_total);
    {
      PhaseScope ps(h, &h->tm.kstar);
      if ((rc = upload_queries<double>(h, Xq, M, mem_kind))) return rc;
    }
    for (int64_t m0 = 0; m0 < Mpad; m0 += MB) {  // query rows are independent: batches change nothing
      const int64_t mp = std::min(MB, Mpad - m0), mv = std::min<int64_t>(mp, M - m0);
      if ((rc = sparse_whiten_queries(h, (const double*)h->scr.Qs.p + m0 * h->d, mv, mp, V1, V2))) return rc;
      sparse_mean_product(h, (double*)h->scr.MT.p + m0, ldm, V2, mp);
      if (var) {
        PhaseScope ps(h, &h->tm.var);
        launch_sparse_var(V1, V2, ld, mv, sp.mpad, h->sf2, 0.0, (double*)h->var.p + m0, h->st);
      }
    }
    {
      PhaseScope ps(h, &h->tm.mean);
      launch_unpack_rhs<double>((const double*)h->scr.MT.p, ldm, M, k, 1.0, (double*)h->meanout.p, h->st);
    }
    if ((rc = deliver_mean_var<double>(h, mean, var, M, mem_kind))) return rc;
  }
  return finish_call(h);
}

int sparse_predict_cov_impl(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* cov, int32_t mem_kind) {
  gpx_handle::Sparse& sp = h->sp;
  const int64_t Mpad = round_up(M, TILE), ldm = Mpad + LD_SKEW, lds = Mpad + LD_SKEW, ld = sp.ld;
  const int k = h->k;
  reset_predict_clocks(h->tm);
  int rc;
  {
    const double need = 8.0 * (2.0 * Mpad * ld + 2.0 * Mpad * lds + (double)RHS_ROWS * ldm + (double)M * k + 2.0 * Mpad * h->d) + 4096;
    const double have = (double)h->scr.SV1.cap + h->scr.SV2.cap + h->scr.SS2.cap + h->scr.JSig.cap;
    size_t freeb = 0, totalb = 0;
    HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
    if (need > (double)freeb + have) {
      char buf[256];
      snprintf(buf, sizeof buf, "gpx_sparse_predict_cov: M = %lld query points need %.3f GB of device memory, %.3f GB are free",
               (long long)M, need / 1e9, ((double)freeb + have) / 1e9);
      return fail(h, GPX_E_NOMEM, buf);
    }
  }
  if ((rc = ensure_queries<double>(h, M))) return rc;
  if ((rc = ensure(h, h->scr.SV1, (size_t)Mpad * ld * 8)) || (rc = ensure(h, h->scr.SV2, (size_t)Mpad * ld * 8))) return rc;
  if ((rc = ensure(h, h->scr.JSig, (size_t)Mpad * lds * 8)) || (rc = ensure(h, h->scr.SS2, (size_t)Mpad * lds * 8))) return rc;
  if ((rc = ensure(h, h->scr.MT, (size_t)RHS_ROWS * ldm * 8))) return rc;
  if ((rc = ensure(h, h->meanout, (size_t)M * k * 8))) return rc;
  double* V1 = (double*)h->scr.SV1.p;
  double* V2 = (double*)h->scr.SV2.p;
  double* dSig = (double*)h->scr.JSig.p;
  double* dS2 = (double*)h->scr.SS2.p;
  {
    PhaseScope total(h, &h->tm.predict_total);
    {
      PhaseScope ps(h, &h->tm.kstar);
      if ((rc = upload_queries<double>(h, Xq, M, mem_kind))) return rc;
    }
    if ((rc = sparse_whiten_queries(h, (const double*)h->scr.Qs.p, M, Mpad, V1, V2))) return rc;
    sparse_mean_product(h, (double*)h->scr.MT.p, ldm, V2, Mpad);
    {
      PhaseScope ps(h, &h->tm.mean);
      launch_unpack_rhs<double>((const double*)h->scr.MT.p, ldm, M, k, 1.0, (double*)h->meanout.p, h->st);
    }
    {  // Sigma = sf2 k(Xs, Xs) - T1^T T1 + T2^T T2 on the lower triangle, mirrored for a bit-symmetric copy-out
      PhaseScope ps(h, &h->tm.var);
      HIPCHK(h, hipMemsetAsync(dSig, 0, (size_t)Mpad * lds * 8, h->st));
      HIPCHK(h, hipMemsetAsync(dS2, 0, (size_t)Mpad * lds * 8, h->st));
      launch_kbuild_sym<double>(h->cfg.kernel, (const double*)h->scr.Qs.p, M, Mpad, h->d, h->sf2, 0.0, dSig, lds, h->st);
      launch_gemm_nt<double>(128, dSig, lds, V1, ld, V1, ld, Mpad, Mpad, sp.mpad, 1, 0, h->st);
      launch_gemm_nt<double>(128, dS2, lds, V2, ld, V2, ld, Mpad, Mpad, sp.mpad, 1, 1, h->st);
      launch_add_block<double>(dSig, lds, dS2, lds, (int)Mpad, (int)Mpad, 1.0, h->st);
      launch_mirror_lower<double>(dSig, lds, Mpad, 0, h->st);
    }
    PhaseScope ps(h, &h->tm.d2h);
    if (mean && (rc = copy_out(h, mean, h->meanout.p, (size_t)M * k * 8, mem_kind))) return rc;
    HIPCHK(h, hipMemcpy2DAsync(cov, (size_t)M * 8, dSig, (size_t)lds * 8, (size_t)M * 8, (size_t)M,
                               mem_kind == GPX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->st));
  }
  return finish_call(h);
}

// The gradient of the bound F = sum_c ELBO_c by the log parameters (lengthscales..., sf2, sn2) of the handle's fit
// (DESIGN.md §3.4r "The gradient of the bound").  With ch = LB^-T c,  H = k (I - B^-1) - ch ch^T  and
// M = k (2 I - B^-1 - B) - ch ch^T:   dF / dKuf^T = T with rows t_n = L^-T (H a_n + ch yt_n^T) / s_n,   dF / dKuu = Guu =
// 1/2 L^-T M L^-1.  Stage 1, O(m^3), all on the tile engine: LB^-T and L^-T by trtri_enqueue, B^-1 = LB^-T LB^-1 and the
// rebuilt B = LB LB^T (the fit's own B was overwritten by its factor, and the fit is not touched), H' = L^-T [H | ch] and
// 2 Guu = (L^-T M) L^-1 as NT products.  Stage 2 streams the observations once more in the fit's own chunks with the fit's
// own launches up to the whitened bordered rows [a_n^T | yt_n^T], forms T = rows H'^T in one NT product per chunk — the ch
// yt^T term rides in the 64 border columns — and contracts T r_n against dKfu / dtheta (launch_cross_dtheta).  The noise
// entry needs no pass: it is a sum of scalars.  Only scratch and the fit's chunk buffers are written: the fit stays as it is.
int sparse_grad_impl(gpx_handle* h, const void* X, const void* y, const void* w, int32_t mem_kind, double* elbo, double* grad) {
  gpx_handle::Sparse& sp = h->sp;
  gpx_handle::ScratchBufs& sc = h->scr;
  const int64_t N = sp.N, m = sp.m, mpad = sp.mpad, nb_ = mpad + RHS_ROWS, ld = sp.ld, C = sp.chunk;
  const int64_t cb = std::min(C, round_up(N, TILE));
  const int d = h->d, k = h->k, n_ls = h->n_ls, nth = n_ls + 1, kernel = h->cfg.kernel;
  const double sf2 = h->sf2, sn2 = h->sn2;
  const int64_t npart = std::max(cross_dtheta_part_elems(cb, mpad, n_ls), cross_dtheta_part_elems(mpad, mpad, n_ls));
  const size_t tail = (size_t)(2 * nth + 2);  // behind the partials: the sums of the Kfu term, of the Kuu term, tr B^-1, |ch|^2
  int rc;
  {  // one more chunk buffer and the m x m temporaries, against what is free plus what the handle holds of them already
    const double need = 8.0 * ((double)nb_ * ld + 4.0 * mpad * ld + (double)cb * ld + (double)npart + (double)tail +
                               (double)cb * (2 * d + k + 1)) + 4096;
    const double have = (double)sc.SGH.cap + sc.SGZ.cap + sc.SGM.cap + sc.SGZL.cap + sc.SGHp.cap + sc.SGT.cap + sc.SGpart.cap +
                        sp.Xc.cap + sp.Xsc.cap + sp.Yc.cap + sp.Wc.cap;
    size_t freeb = 0, totalb = 0;
    HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
    if (need > (double)freeb + have) {
      char buf[256];
      snprintf(buf, sizeof buf, "gpx_sparse_elbo_grad: m = %lld inducing points with chunks of %lld rows need %.3f GB more of "
               "device memory, %.3f GB are free", (long long)m, (long long)cb, need / 1e9, ((double)freeb + have) / 1e9);
      return fail(h, GPX_E_NOMEM, buf);
    }
  }
  if ((rc = ensure(h, sc.SGH, (size_t)nb_ * ld * 8)) || (rc = ensure(h, sc.SGZ, (size_t)mpad * ld * 8)) ||
      (rc = ensure(h, sc.SGM, (size_t)mpad * ld * 8)) || (rc = ensure(h, sc.SGZL, (size_t)mpad * ld * 8)) ||
      (rc = ensure(h, sc.SGHp, (size_t)mpad * ld * 8)) || (rc = ensure(h, sc.SGT, (size_t)cb * ld * 8)) ||
      (rc = ensure(h, sc.SGpart, ((size_t)npart + tail) * 8)))
    return rc;
  if ((rc = ensure(h, sp.Xc, (size_t)cb * d * 8)) || (rc = ensure(h, sp.Xsc, (size_t)cb * d * 8)) ||
      (rc = ensure(h, sp.Yc, (size_t)cb * k * 8)) || (w && (rc = ensure(h, sp.Wc, (size_t)cb * 8))))
    return rc;
  double* GH = (double*)sc.SGH.p;    // [H | ch^T]: mpad rows of B^-1, then H; ch^T in the 64 rows below
  double* GZ = (double*)sc.SGZ.p;    // LB^-T, then LB with a zero upper triangle, then L^-T M
  double* GM = (double*)sc.SGM.p;    // B rebuilt, then M, then 2 Guu
  double* GZL = (double*)sc.SGZL.p;  // L^-T
  double* GHp = (double*)sc.SGHp.p;  // H' = L^-T [H | ch] (mpad x nb_)
  double* GT = (double*)sc.SGT.p;    // T of one chunk
  double* part = (double*)sc.SGpart.p;
  double* accx = part + npart;
  double* accu = accx + nth;
  double* gsc = accu + nth;
  double* chT = GH + mpad * ld;
  const double* dL = (const double*)sp.L.p;
  const double* dB = (const double*)sp.B.p;
  const double* dZs = (const double*)sp.Zs.p;
  double* dKc = (double*)sp.Kc.p;
  gpx_timings& tm = h->tm;
  tm.grad_trtri = tm.grad_trace = tm.grad_total = 0;
  hipStream_t st = h->st;
  {
    PhaseScope total(h, &tm.grad_total);
    {
      PhaseScope ps(h, &tm.grad_trtri);
      HIPCHK(h, hipMemsetAsync(accx, 0, tail * 8, st));
      HIPCHK(h, hipMemsetAsync(GZ, 0, (size_t)mpad * ld * 8, st));
      launch_set_diag_one(GZ, ld, mpad, st);
      if ((rc = trtri_enqueue(h, GZ, dB, ld, mpad, SP_NB, (const double*)sp.WinvB.p, 1, 0))) return rc;
      HIPCHK(h, hipMemsetAsync(GH, 0, (size_t)nb_ * ld * 8, st));
      launch_gemm_nt<double>(64, chT, ld, dB + mpad * ld, ld, GZ, ld, RHS_ROWS, mpad, mpad, 0, 1, st);  // ch^T = c^T LB^-1
      launch_gemm_nt<double>(128, GH, ld, GZ, ld, GZ, ld, mpad, mpad, mpad, 0, 1, st);                  // B^-1
      launch_sparse_grad_scalars(GH, ld, mpad, chT, k, gsc, st);
      launch_copy_lower<double>(GZ, ld, dB, ld, mpad, st);
      launch_mirror_lower<double>(GZ, ld, mpad, 1, st);
      launch_gemm_nt<double>(128, GM, ld, GZ, ld, GZ, ld, mpad, mpad, mpad, 0, 1, st);  // B = LB LB^T
      launch_sparse_grad_weights(GH, GM, ld, mpad, chT, k, st);
      HIPCHK(h, hipMemsetAsync(GZL, 0, (size_t)mpad * ld * 8, st));
      launch_set_diag_one(GZL, ld, mpad, st);
      if ((rc = trtri_enqueue(h, GZL, dL, ld, mpad, SP_NB, (const double*)sp.WinvL.p, 1, 0))) return rc;
      launch_gemm_nt<double>(64, GHp, ld, GZL, ld, GH, ld, mpad, nb_, mpad, 0, 1, st);
      launch_gemm_nt<double>(128, GZ, ld, GZL, ld, GM, ld, mpad, mpad, mpad, 0, 1, st);  // L^-T M (M is symmetric)
      launch_gemm_nt<double>(128, GM, ld, GZ, ld, GZL, ld, mpad, mpad, mpad, 0, 1, st);  // 2 Guu
      launch_cross_dtheta(kernel, GM, ld, m, mpad, m, mpad, dZs, dZs, d, n_ls, sf2, nullptr, 1.0, part, accu, st);
    }
    PhaseScope ps(h, &tm.grad_trace);
    for (int64_t c0 = 0; c0 < N; c0 += C) {  // the fit's chunks, the fit's launches up to the whitened rows
      const int64_t rows = std::min(C, N - c0), rp = round_up(rows, TILE);
      if ((rc = copy_in(h, sp.Xc.p, (const double*)X + c0 * d, (size_t)rows * d * 8, mem_kind))) return rc;
      if ((rc = copy_in(h, sp.Yc.p, (const double*)y + c0 * k, (size_t)rows * k * 8, mem_kind))) return rc;
      if (w && (rc = copy_in(h, sp.Wc.p, (const double*)w + c0, (size_t)rows * 8, mem_kind))) return rc;
      launch_scale_points<double>((const double*)sp.Xc.p, rows, rp, d, (const double*)h->ls.p, n_ls, (double*)sp.Xsc.p, st);
      launch_kbuild_cross<double>(kernel, (const double*)sp.Xsc.p, rows, rp, dZs, m, mpad, d, sf2, dKc, ld, st);
      launch_sparse_border(dKc, ld, rows, rp, mpad, (const double*)sp.Yc.p, k, w ? (const double*)sp.Wc.p : nullptr, sn2, st);
      if ((rc = solve_fwd_enqueue<double>(h, dKc, rp, dL, ld, mpad, SP_NB, (const double*)sp.WinvL.p))) return rc;
      launch_gemm_nt<double>(128, GT, ld, dKc, ld, GHp, ld, rp, mpad, nb_, 0, 1, st);
      launch_cross_dtheta(kernel, GT, ld, rows, rp, m, mpad, (const double*)sp.Xsc.p, dZs, d, n_ls, sf2,
                          w ? (const double*)sp.Wc.p : nullptr, sn2, part, accx, st);
    }
  }
  double scal[32], sums[2 * (MAX_D + 1) + 2];
  HIPCHK(h, hipMemcpyAsync(scal, sp.scal.p, sizeof scal, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(sums, accx, tail * 8, hipMemcpyDeviceToHost, st));
  if ((rc = finish_call(h))) return rc;
  const double kk = (double)k, inv = sp.sum_inv_s2;
  double yy = 0.0, cc = 0.0;
  for (int c = 0; c < k; ++c) yy += scal[1 + c], cc += scal[17 + c];
  for (int t = 0; t < nth; ++t) grad[t] = sums[t] + 0.5 * sums[nth + t];
  grad[n_ls] -= 0.5 * kk * sf2 * inv;
  const double trBinv_pad = sums[2 * nth], chch = sums[2 * nth + 1];  // (the mpad - m padded rows of B^-1 add one each)
  grad[n_ls + 1] = 0.5 * kk * ((double)mpad - trBinv_pad) - 0.5 * kk * (double)N + 0.5 * yy - cc + 0.5 * (cc - chch) +
                   0.5 * kk * sf2 * inv - 0.5 * kk * scal[0];
  if (elbo) std::copy(sp.elbo, sp.elbo + k, elbo);
  return GPX_OK;
}

}  // namespace
}  // extern "C++"

int gpx_sparse_fit(gpx_handle* h, const void* X, const void* y, const void* w, int64_t N, int32_t d, int32_t k, const void* Z,
                   int64_t m, const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter, int64_t chunk,
                   int32_t mem_kind, int64_t* info) try {
  const char* fn = "gpx_sparse_fit";
  if (!h) return GPX_E_ARG;
  auto bad = [&](const char* what) { return fail(h, GPX_E_ARG, fn, what); };
  if (!X || !y || !Z || !lengthscale || !info) return bad("null argument");
  if (N <= 0 || m <= 0 || d <= 0 || d > MAX_D) return bad("need N > 0, m > 0 and 1 <= d <= 32");
  if (k <= 0 || k > SP_MAX_K) return bad("need 1 <= k <= 8 target columns");
  if (n_ls != 1 && n_ls != d) return bad("n_ls must be 1 or d");
  if (bad_mem_kind(mem_kind)) return bad("bad mem_kind");
  if (!(sf2 > 0.0) || !(sn2 > 0.0) || !(jitter >= 0.0) || !std::isfinite(sf2) || !std::isfinite(sn2) || !std::isfinite(jitter))
    return bad("need finite sf2 > 0, sn2 > 0, jitter >= 0");
  for (int i = 0; i < n_ls; ++i)
    if (!(lengthscale[i] > 0.0) || !std::isfinite(lengthscale[i])) return bad("lengthscale must be finite and > 0");
  if (chunk < 0 || chunk > ((int64_t)1 << 24)) return bad("need 0 <= chunk <= 2^24");
  if (N > ((int64_t)1 << 40) || m > 65536) return bad("N or m too large (m <= 65536)");
  int rc;
  if ((rc = sparse_handle_refused(h, fn))) return rc;
  if ((rc = begin_call(h))) return rc;
  // the weights, on the host: each finite and > 0; sum log s_n^2 and sum 1 / s_n^2 in index order
  double sum_log_s2 = (double)N * std::log(sn2), sum_inv_s2 = (double)N / sn2;
  if (w) {
    std::vector<double> tmp;
    const double* hw = (const double*)w;
    if (mem_kind == GPX_MEM_DEVICE) {
      tmp.resize((size_t)N);
      HIPCHK(h, hipMemcpy(tmp.data(), w, (size_t)N * 8, hipMemcpyDeviceToHost));
      hw = tmp.data();
    }
    sum_log_s2 = sum_inv_s2 = 0.0;
    for (int64_t i = 0; i < N; ++i) {
      if (!(hw[i] > 0.0) || !std::isfinite(hw[i]))
        return bad("noise weights must be finite and > 0 (a waypoint, w = 0, has no place in S^-1)");
      sum_log_s2 += std::log(sn2 * hw[i]);
      sum_inv_s2 += 1.0 / (sn2 * hw[i]);
    }
  }
  // this call replaces whatever fit the handle holds; a dense factor leaves the device with it
  HIPCHK(h, hipDeviceSynchronize());
  h->fitted = false;
  h->sp.fitted = false;
  h->basis = h->bp = 0;
  h->pw = {};
  h->K = {}, h->P = {}, h->Wblk = {}, h->Lfull = {}, h->AT = {};
  h->zT = h->alphaT = nullptr, h->Lfac = nullptr, h->alpha_ready = false, h->nbw = 0;
  return sparse_fit_impl(h, X, y, w, N, d, k, Z, m, lengthscale, n_ls, sf2, sn2, jitter, chunk, mem_kind, sum_log_s2, sum_inv_s2, info);
}
GPX_CATCH_ALL

int gpx_sparse_predict(gpx_handle* h, const void* Xs, int64_t M, void* mean, void* var, int32_t mem_kind) try {
  const char* fn = "gpx_sparse_predict";
  if (!h) return GPX_E_ARG;
  int rc;
  if ((rc = sparse_handle_refused(h, fn)) || (rc = sparse_unfitted(h, fn))) return rc;
  if (!Xs || !mean || M <= 0 || M > (int64_t)INT_MAX - 4096) return fail(h, GPX_E_ARG, fn, "bad argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, fn, "bad mem_kind");
  if ((rc = begin_call(h))) return rc;
  return sparse_predict_impl(h, Xs, M, mean, var, mem_kind);
}
GPX_CATCH_ALL

int gpx_sparse_predict_cov(gpx_handle* h, const void* Xs, int64_t M, void* mean, void* cov, int32_t mem_kind) try {
  const char* fn = "gpx_sparse_predict_cov";
  if (!h) return GPX_E_ARG;
  int rc;
  if ((rc = sparse_handle_refused(h, fn)) || (rc = sparse_unfitted(h, fn))) return rc;
  if (!Xs || !cov || M <= 0 || M > 1000000) return fail(h, GPX_E_ARG, fn, "bad argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, fn, "bad mem_kind");
  if ((rc = begin_call(h))) return rc;
  return sparse_predict_cov_impl(h, Xs, M, mean, cov, mem_kind);
}
GPX_CATCH_ALL

int gpx_sparse_elbo(gpx_handle* h, double* elbo) try {
  if (!h) return GPX_E_ARG;
  int rc;
  if ((rc = sparse_handle_refused(h, "gpx_sparse_elbo")) || (rc = sparse_unfitted(h, "gpx_sparse_elbo"))) return rc;
  if (!elbo) return fail(h, GPX_E_ARG, "gpx_sparse_elbo", "null output");
  std::copy(h->sp.elbo, h->sp.elbo + h->k, elbo);
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_sparse_info(gpx_handle* h, int64_t* N, int64_t* m, int64_t* k, int64_t* chunk) try {
  if (!h) return GPX_E_ARG;
  int rc;
  if ((rc = sparse_handle_refused(h, "gpx_sparse_info")) || (rc = sparse_unfitted(h, "gpx_sparse_info"))) return rc;
  if (N) *N = h->sp.N;
  if (m) *m = h->sp.m;
  if (k) *k = h->k;
  if (chunk) *chunk = h->sp.chunk;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_sparse_elbo_grad(gpx_handle* h, const void* X, const void* y, const void* w, int64_t N, int32_t mem_kind, double* elbo,
                         double* grad) try {
  const char* fn = "gpx_sparse_elbo_grad";
  if (!h) return GPX_E_ARG;
  int rc;
  if ((rc = sparse_handle_refused(h, fn)) || (rc = sparse_unfitted(h, fn))) return rc;
  if (!X || !y || !grad) return fail(h, GPX_E_ARG, fn, "null argument");
  if (bad_mem_kind(mem_kind)) return fail(h, GPX_E_ARG, fn, "bad mem_kind");
  if (N != h->sp.N) return fail(h, GPX_E_ARG, fn, "N differs from the fit's: pass the observations the handle was fitted to");
  if ((rc = begin_call(h))) return rc;
  return sparse_grad_impl(h, X, y, w, mem_kind, elbo, grad);
}
GPX_CATCH_ALL

int gpx_cross_dtheta_contract(int32_t kernel, const double* A, int64_t na, const double* B, int64_t nb_, int32_t d,
                              const double* W, const double* lengthscale, int32_t n_ls, double sf2, double* out) try {
  if (!A || !B || !W || !out || !lengthscale || !sizes_ok(na, nb_, d, n_ls) || !cov::known(kernel)) return GPX_E_ARG;
  if (na > ((int64_t)1 << 20) || nb_ > ((int64_t)1 << 20) || round_up(na, 64) * round_up(nb_, 64) > ((int64_t)1 << 28))
    return GPX_E_ARG;
  KernelCall<double> kc;
  if (int rc = kc.points(A, na, B, nb_, d, lengthscale, n_ls)) return rc;
  const int64_t ldw = kc.nbpad, npart = cross_dtheta_part_elems(kc.napad, kc.nbpad, n_ls);
  Dev<double> dW, dPart;
  if (int rc; (rc = dW.alloc((size_t)kc.napad * ldw)) || (rc = dPart.alloc((size_t)npart + n_ls + 1))) return rc;
  double* acc = dPart + npart;
  UCHK(hipMemsetAsync(dW, 0, (size_t)kc.napad * ldw * 8, kc.st));
  UCHK(hipMemsetAsync(acc, 0, (size_t)(n_ls + 1) * 8, kc.st));
  UCHK(hipMemcpy2DAsync(dW, (size_t)ldw * 8, W, (size_t)nb_ * 8, (size_t)nb_ * 8, (size_t)na, hipMemcpyHostToDevice, kc.st));
  launch_cross_dtheta(kernel, dW, ldw, na, kc.napad, nb_, kc.nbpad, kc.As, kc.Bs, d, n_ls, sf2, nullptr, 1.0, dPart, acc, kc.st);
  std::vector<double> res((size_t)n_ls + 1);
  UCHK(hipMemcpyAsync(res.data(), acc, res.size() * 8, hipMemcpyDeviceToHost, kc.st));
  if (int rc = kc.sc.finish()) return rc;
  std::copy(res.begin(), res.end(), out);
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_syrk_tn(double* C, int64_t n, const double* X, int64_t rows, int32_t accumulate) try {
  if (!C || !X || n <= 0 || n % 64 != 0 || n > 16384 || rows <= 0 || rows > ((int64_t)1 << 24)) return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const int64_t ld = n + LD_SKEW;
  Dev<double> dC, dX, dPart;
  if (int rc; (rc = dC.alloc((size_t)n * ld)) || (rc = dX.alloc((size_t)rows * ld)) ||
              (rc = dPart.alloc((size_t)syrk_tn_part_elems(n, rows))))
    return rc;
  UCHK(hipMemcpy2DAsync(dC, (size_t)ld * 8, C, (size_t)n * 8, (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice, sc.st));
  UCHK(hipMemcpy2DAsync(dX, (size_t)ld * 8, X, (size_t)n * 8, (size_t)n * 8, (size_t)rows, hipMemcpyHostToDevice, sc.st));
  launch_syrk_tn(dC, ld, n, dX, ld, rows, rows, dPart, accumulate != 0, sc.st);
  UCHK(hipMemcpy2DAsync(C, (size_t)n * 8, dC, (size_t)ld * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost, sc.st));
  return sc.finish();
}
GPX_CATCH_ALL

// The contraction of the inducing-point fit alone, operands resident and zero-filled: C (n x n, lower) += X^T X for X
// (rows x n), `iters` back-to-back repeats after one warm-up; *ms = mean time of one.  route 0: the TN kernel as the fit
// launches it (partials + reduction); route 1: a transpose of X followed by the NT tile engine on 128-tiles (what the fit
// would do instead of the TN kernel); route 2: that NT launch alone (gpx_debug_gemm_bench's, for the engine's own rate).
int gpx_debug_syrk_tn_bench(int64_t n, int64_t rows, int32_t route, int32_t iters, double* ms_per_call) try {
  if (!ms_per_call || n <= 0 || n % 128 || n > 16384 || rows <= 0 || rows % 64 || rows > ((int64_t)1 << 22) || iters <= 0 ||
      route < 0 || route > 2)
    return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const int64_t ldc = n + LD_SKEW, ldx = n + LD_SKEW, ldt = rows + LD_SKEW;
  Dev<double> dC, dX, dXT, dPart;
  float t = 0.f;
  if (int rc; (rc = dC.alloc((size_t)n * ldc)) || (rc = dX.alloc((size_t)rows * ldx)) || (rc = dXT.alloc((size_t)n * ldt)) ||
              (rc = dPart.alloc((size_t)syrk_tn_part_elems(n, rows))))
    return rc;
  UCHK(hipMemsetAsync(dC, 0, (size_t)n * ldc * 8, sc.st));
  UCHK(hipMemsetAsync(dX, 0, (size_t)rows * ldx * 8, sc.st));
  UCHK(hipMemsetAsync(dXT, 0, (size_t)n * ldt * 8, sc.st));
  hipEvent_t e0 = next_event(&sc.h), e1 = next_event(&sc.h);
  if (!e0 || !e1) return fail(nullptr, GPX_E_HIP, "hipEventCreate failed");
  auto once = [&] {
    if (route == 0) {
      launch_syrk_tn(dC, ldc, n, dX, ldx, rows, rows, dPart, 1, sc.st);
      return;
    }
    if (route == 1) launch_transpose(dX, ldx, rows, n, dXT, ldt, sc.st);
    launch_gemm_nt_fixed<double>(128, dC, ldc, dXT, ldt, dXT, ldt, n, n, rows, 1, 0, sc.st);
  };
  once();
  UCHK(hipEventRecord(e0, sc.st));
  for (int i = 0; i < iters; ++i) once();
  UCHK(hipEventRecord(e1, sc.st));
  if (int rc = sc.finish()) return rc;
  UCHK(hipEventElapsedTime(&t, e0, e1));
  *ms_per_call = (double)t / iters;
  return GPX_OK;
}
GPX_CATCH_ALL

// The derivative contraction of the bound's gradient alone, operands resident and zero-filled: W (rows x cols at the fit's
// leading dimension cols + 64 + skew) against rows x cols points of d dimensions, n_ls lengthscales, `iters` back-to-back
// repeats after one warm-up; *ms = mean time of one (the kernel and its reduction).  rows, cols multiples of 64.
int gpx_debug_cross_dtheta_bench(int32_t kernel, int64_t rows, int64_t cols, int32_t d, int32_t n_ls, int32_t iters,
                                 double* ms_per_call) try {
  if (!ms_per_call || !cov::known(kernel) || !sizes_ok(rows, cols, d, n_ls) || rows % 64 || cols % 64 || rows > ((int64_t)1 << 22) ||
      cols > 65536 || iters <= 0)
    return GPX_E_ARG;
  Scratch sc;
  if (!sc.ok) return GPX_E_HIP;
  const int64_t ldw = cols + RHS_ROWS + LD_SKEW, npart = cross_dtheta_part_elems(rows, cols, n_ls);
  Dev<double> dW, dA, dB, dPart;
  float t = 0.f;
  if (int rc; (rc = dW.alloc((size_t)rows * ldw)) || (rc = dA.alloc((size_t)rows * d)) || (rc = dB.alloc((size_t)cols * d)) ||
              (rc = dPart.alloc((size_t)npart + n_ls + 1)))
    return rc;
  UCHK(hipMemsetAsync(dW, 0, (size_t)rows * ldw * 8, sc.st));
  UCHK(hipMemsetAsync(dA, 0, (size_t)rows * d * 8, sc.st));
  UCHK(hipMemsetAsync(dB, 0, (size_t)cols * d * 8, sc.st));
  UCHK(hipMemsetAsync(dPart, 0, ((size_t)npart + n_ls + 1) * 8, sc.st));
  hipEvent_t e0 = next_event(&sc.h), e1 = next_event(&sc.h);
  if (!e0 || !e1) return fail(nullptr, GPX_E_HIP, "hipEventCreate failed");
  auto once = [&] {
    launch_cross_dtheta(kernel, dW, ldw, rows, rows, cols, cols, dA, dB, d, n_ls, 1.0, nullptr, 1.0, dPart, dPart + npart, sc.st);
  };
  once();
  UCHK(hipEventRecord(e0, sc.st));
  for (int i = 0; i < iters; ++i) once();
  UCHK(hipEventRecord(e1, sc.st));
  if (int rc = sc.finish()) return rc;
  UCHK(hipEventElapsedTime(&t, e0, e1));
  *ms_per_call = (double)t / iters;
  return GPX_OK;
}
GPX_CATCH_ALL
