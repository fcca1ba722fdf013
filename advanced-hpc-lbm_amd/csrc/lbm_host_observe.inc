// lbm_host_observe.inc -- part of lbm_api.hip (included there): lbm_run_observed, one run with any subset of the four
// observers (forces, probes, means, snapshots).  DESIGN.md 3.11.
//
// One observer alone IS its own call.  Two or more: the step loop is cut into pieces at the sample steps of the observers that
// are not taken inside a launch -- means and snapshots always; probes where the register tiles do not run -- and each piece is
// one run_steps with a RunKind that carries the observers taken inside it.
//   register tiles   EVERY piece runs the kRegForce | kRegProbe flavour (RunKind::piece), whichever of the two is wanted: it
//            alone knows a first-sample phase (pfirst), and it alone folds the last step's speed sum of a piece that is not the
//            call's last as the loop folds every other step's (piece_mid) -- a whole-run launch folds its last step in
//            another order of additions, so pieces of the other flavours would move the last bit of av_vels at the cuts.
//            An observer that is not wanted gets the table of -1s.  A piece of n steps leaves its forces behind its per-step
//            sums (sums + n + 1), reduced and fetched with them.
//   elsewhere        forces as lbm_run_forces there (one-step kernel, lbm_body_forces behind each step), lbm_probe_gather
//            behind the piece that ends on a probe sample step.
// Behind a piece, on the slabs' streams: lbm_mean_add into the per-slab sums, lbm_final_state's derive into the snapshot's
// slot.  lbm_mean_div and the copies of staged output to the host after the last piece.
// A register-tile piece that gives up (or whose flavour is not resident) has stepped nothing: run_steps says so (RunKind::ran),
// and the loop repeats THAT piece from the same `done` off the tiles (RunKind::no_tiles, for the rest of the call) -- cut at
// the probes' sample steps, every row of the piece gathered again, the forces of its steps stored again.
namespace {

// a piece's forces: the local slabs' sums behind its per-step sums (a rank: everybody's, through the all-reduce that ended it)
void observed_forces(const lbm_ctx* c, int n, long nval, float* out) {
  for (long k = 0; k < nval; ++k) {
    double acc = 0.0;
    for (auto& s : c->slabs) acc += s.sums_host[n + 1 + k];
    out[k] = (float)acc;
  }
}

// the table of -1s of a slab for the current tiling (LBM_ENOMEM: nothing queued)
int observed_no_force_table(Slab& s, int ntiles) {
  if (s.fslot_none && s.fslot_none_n == ntiles) return LBM_OK;
  HIPC(hipSetDevice(s.dev));
  if (s.fslot_none) HIPC(hipFree(s.fslot_none));
  s.fslot_none = nullptr; s.fslot_none_n = 0;
  if (hipMalloc((void**)&s.fslot_none, sizeof(int) * (size_t)ntiles) != hipSuccess) {
    (void)hipGetLastError();
    s.fslot_none = nullptr;
    return fail(LBM_ENOMEM, "no room on device %d for the empty force table (%d tiles)", s.dev, ntiles);
  }
  HIPC(hipMemset(s.fslot_none, 0xff, sizeof(int) * (size_t)ntiles));
  s.fslot_none_n = ntiles;
  return LBM_OK;
}

}  // namespace

static_assert(sizeof(lbm_observe) == 48 && offsetof(lbm_observe, forces) == 0 && offsetof(lbm_observe, probes_out) == 8 &&
              offsetof(lbm_observe, mean_out) == 16 && offsetof(lbm_observe, fields_out) == 24 && offsetof(lbm_observe, probes_every) == 32 &&
              offsetof(lbm_observe, mean_every) == 36 && offsetof(lbm_observe, fields_every) == 40, "the layout lbm_mi355x.h states");

extern "C" int lbm_run_observed(lbm_ctx* c, int nsteps, float* av_vels, const lbm_observe* what) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  const bool wf = what && what->forces, wp = what && what->probes_out, wm = what && what->mean_out;
  bool ws = what && what->fields_out;
  const int pe = wp ? what->probes_every : 0, me = wm ? what->mean_every : 0, se = ws ? what->fields_every : 0;
  // ---- refusals: nothing queued, the lattice untouched
  if (wf && c->nbodies == 0) return fail(LBM_EINVAL, "forces are wanted but no bodies are set (lbm_set_bodies)");
  if (wp && c->nprobes == 0) return fail(LBM_EINVAL, "probes are wanted but no probes are set (lbm_set_probes)");
  if (wp && pe <= 0) return fail(LBM_EINVAL, "probes_every must be positive (got %d)", pe);
  if (wp && nsteps / pe == 0) return fail(LBM_EINVAL, "nothing to record: no sample step in nsteps = %d step(s) at probes_every = %d", nsteps, pe);
  if (wm && me <= 0) return fail(LBM_EINVAL, "mean_every must be positive (got %d)", me);
  if (wm && nsteps / me == 0) return fail(LBM_EINVAL, "nothing to average: no sample step in %d step(s) at mean_every = %d", nsteps, me);
  if (ws && se < 0) return fail(LBM_EINVAL, "fields_every < 0");
  const int mp = wp ? nsteps / pe : 0, mm = wm ? nsteps / me : 0, msn = (ws && se > 0) ? nsteps / se : 0;
  if (msn == 0) ws = false;                               // (no snapshot is due: legal, nothing written, as lbm_run_sampled)
  if (c->p2p_failed) return fail(LBM_EHIP, "a peer-to-peer halo wait timed out earlier: this lattice is no longer defined");
  bool p_dev = false, m_dev = false, s_dev = false;
  int rc;
  if (wp && (rc = output_on_device(c, what->probes_out, "probes_out", &p_dev))) return rc;
  if (wm && (rc = output_on_device(c, what->mean_out, "mean_out", &m_dev))) return rc;
  if (ws && (rc = output_on_device(c, what->fields_out, "fields_out", &s_dev))) return rc;
  c->observed_in_kernel = 0; c->observed_in_wave = 0; c->observed_pieces = 0;
  if (wf) c->forces_in_wave = 0;                          // (set by any piece whose forces rode in lbm_wave launches)
  // ---- none, or one alone: the call itself
  const int wanted = (wf ? 1 : 0) + (wp ? 1 : 0) + (wm ? 1 : 0) + (ws ? 1 : 0);
  if (wanted <= 1) {
    if (wf) { rc = lbm_run_forces(c, nsteps, av_vels, what->forces); if (!rc && c->forces_in_kernel) c->observed_in_kernel = 1; if (!rc && c->forces_in_wave) c->observed_in_wave = 1; }
    else if (wp) { rc = lbm_run_probes(c, nsteps, av_vels, pe, what->probes_out); if (!rc && c->probes_in_kernel) c->observed_in_kernel = 2; if (!rc && c->probes_in_wave) c->observed_in_wave = 2; }
    else if (wm) { rc = lbm_run_mean(c, nsteps, av_vels, me, what->mean_out); if (!rc && c->mean_in_kernel) c->observed_in_kernel = 4; }
    else if (ws) { rc = lbm_run_sampled(c, nsteps, av_vels, se, what->fields_out); if (!rc && c->samples_in_kernel) c->observed_in_kernel = 8; }
    else rc = lbm_run(c, nsteps, av_vels);
    if (!rc) {
      const int m = wp ? mp : wm ? mm : ws ? msn : 0, ev = wp ? pe : wm ? me : se;
      // (a lone mean or snapshot series that rode in lbm_wave launches ran in one piece too; observed_in_wave keeps its two bits)
      const bool fields_in_wave = (wm && c->mean_in_wave) || (ws && c->samples_in_wave);
      c->observed_pieces = (wanted == 0 || wf || c->observed_in_kernel != 0 || c->observed_in_wave != 0 || fields_in_wave) ? 1 : m + (nsteps > m * ev ? 1 : 0);
    }
    return rc;
  }
  // ---- two or more.  Everything that can fail for want of room is decided here, before anything is queued.
  const int nx = c->p.nx, nb = c->nbodies, np = c->nprobes;
  const size_t ns = c->slabs.size();
  const int base_row = c->rank_mode ? c->slabs[0].row0 : 0;
  long rows = 0;
  for (auto& s : c->slabs) rows += s.nyl;
  const long slot = rows * nx * 4;                        // floats per snapshot
  if (ws && (unsigned long long)msn > (unsigned long long)(PTRDIFF_MAX / 4) / (unsigned long long)slot)
    return fail(LBM_EINVAL, "%d snapshots of %ld floats do not fit the address space", msn, slot);
  if (wf && 2L * nb * nsteps + nsteps + 1 > (1L << 30)) return fail(LBM_EINVAL, "a forces run of %d steps is too long (split it)", nsteps);
  bool tiles = regtile_is_next(c);
  const size_t pfloat = 4 * (size_t)mp * (size_t)np;
  std::vector<DeviceTemp> pstage(ns), macc(ns);
  size_t plocal = 0;
  rc = LBM_OK;
  for (size_t i = 0; i < ns && !rc; ++i) {
    Slab& s = c->slabs[i];
    HIPC(hipSetDevice(s.dev));
    if (wf && ensure_sums(s, (int)(nsteps + 1 + 2L * nb * nsteps))) {
      (void)hipGetLastError();
      rc = fail(LBM_ENOMEM, "no room for the sums of %d steps and their forces", nsteps);
    }
    if (!rc && tiles && !(wf && wp)) rc = observed_no_force_table(s, c->tplan.ntx * c->tplan.nty);
    if (!rc && wf && tiles) rc = force_tables(c, s, c->tplan.ty, c->tplan.ntx, nsteps);
    if (wp) plocal += s.pcells_host.size();
    if (!rc && wp && !p_dev && !s.pcells_host.empty() && hipMalloc(&pstage[i].p, sizeof(float) * pfloat) != hipSuccess) {
      (void)hipGetLastError();
      pstage[i].p = nullptr;
      rc = fail(LBM_ENOMEM, "no room on device %d for %d sample(s) of %d probe(s) of slab %zu (%zu bytes)", s.dev, mp, np, i, sizeof(float) * pfloat);
    }
    if (!rc && wp && tiles) rc = probe_tables(c, s, c->tplan.ty, c->tplan.ntx);
    if (!rc && wm && hipMalloc(&macc[i].p, sizeof(float) * 4 * (size_t)s.nyl * (size_t)nx) != hipSuccess) {
      (void)hipGetLastError();
      macc[i].p = nullptr;
      rc = fail(LBM_ENOMEM, "no room on device %d for the sums of slab %zu (%zu bytes)", s.dev, i, sizeof(float) * 4 * (size_t)s.nyl * (size_t)nx);
    }
  }
  if ((rc = ranks_agree(c, rc, &tiles, "the observers' buffers"))) return rc;
  // probes where lbm_run would run lbm_wave (a lattice alone): they ride in its launches, beside the forces if those are
  // wanted, and cut no piece; decided here, before anything is queued (no: lbm_probe_gather behind pieces cut at their steps)
  const bool pwave = wp && !rc && !tiles && wave_probes_admit(c, wf);
  int wbits = 0;
  // the probes of other ranks' rows read +0.0f
  if (wp && plocal < (size_t)np) {
    if (p_dev) {
      Slab& s = c->slabs[0];
      HIPC(hipSetDevice(s.dev));
      HIPC(hipMemsetAsync(what->probes_out, 0, sizeof(float) * pfloat, s.sc));
      HIPC(hipStreamSynchronize(s.sc));
    } else memset(what->probes_out, 0, sizeof(float) * pfloat);
  }
  auto probes_of = [&](size_t i) { return p_dev ? what->probes_out : (float*)pstage[i].p; };
  auto mean_of = [&](size_t i) { return m_dev ? what->mean_out + 4L * (c->slabs[i].row0 - base_row) * nx : (float*)macc[i].p; };
  if (wm)
    for (size_t i = 0; i < ns; ++i) {
      Slab& s = c->slabs[i];
      HIPC(hipSetDevice(s.dev));
      HIPC(hipMemsetAsync(macc[i].p, 0, sizeof(float) * 4 * (size_t)s.nyl * (size_t)nx, s.sc));
    }
  // ---- the pieces
  double gpu_ms = 0.0, wall_ms = 0.0;
  int done = 0, pieces = 0, bits = 0, jsnap = 0;
  while (done < nsteps) {
    const bool on_tiles = tiles && regtile_is_next(c);
    int next = nsteps;
    if (wm) next = std::min<long>(next, ((long)done / me + 1) * me);
    if (ws) next = std::min<long>(next, ((long)done / se + 1) * se);
    if (wp && !on_tiles && !pwave) next = std::min<long>(next, ((long)done / pe + 1) * pe);
    const int n = next - done;
    const long nval = wf ? 2L * nb * n : 0;
    const int jp = wp ? done / pe : 0;                    // the probes' samples taken before this piece
    float* av = av_vels ? av_vels + done : nullptr;
    RunKind k;
    if (wf) { k.nb = nb; k.nval = nval; k.force_tiles = on_tiles; }
    if (on_tiles) {
      SnapPlan sp;
      sp.every = pe;
      for (size_t i = 0; wp && i < ns; ++i) {
        float* at = probes_of(i);
        sp.at.push_back(at ? at + 4 * (size_t)jp * (size_t)np : nullptr);   // (a slab without a probe stores nothing)
        sp.stride.push_back(4L * np);
      }
      bool ran = false;
      if (wp) { k.snap = &sp; k.probe = true; k.pfirst = pe - done % pe; }
      k.piece = true; k.piece_mid = next < nsteps; k.ran = &ran;
      if ((rc = run_steps(c, n, av, k))) return rc;
      if (!ran) { tiles = false; continue; }              // (nothing stepped: this piece again, off the tiles)
      bits |= (wf ? 1 : 0) | (wp ? 2 : 0);
    } else {
      k.no_tiles = true;
      if (pwave) {
        // (the probes' phase runs on from the start of the call: the first sample of this piece, and its row of the output)
        k.wave_pevery = pe; k.pfirst = pe - done % pe; k.wave_pout = probes_of(0) + 4 * (size_t)jp * (size_t)np;
        c->probes_in_wave = 0;
      }
      if ((rc = run_steps(c, n, av, k))) return rc;
      if (pwave && c->probes_in_wave) wbits |= 2;
      if (wf && c->forces_in_wave) wbits |= 1;
      if (wp && !pwave && (done + n) % pe == 0)
        for (size_t i = 0; i < ns; ++i) {
          Slab& s = c->slabs[i];
          const int n_here = (int)s.pcells_host.size();
          if (n_here == 0) continue;
          HIPC(hipSetDevice(s.dev));
          hipLaunchKernelGGL(lbm::lbm_probe_gather, dim3(cdiv(n_here, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc, s.lat[c->cur], s.plane,
                             s.pcells, n_here, s.blocked, c->p.density, probes_of(i) + 4 * (size_t)jp * (size_t)np);
          HIPC(hipGetLastError());
        }
    }
    if (wf) observed_forces(c, n, nval, what->forces + 2L * nb * done);
    gpu_ms += c->gpu_ms; wall_ms += c->wall_ms;
    done += n;
    ++pieces;
    if (wm && done % me == 0)
      for (size_t i = 0; i < ns; ++i) {
        Slab& s = c->slabs[i];
        HIPC(hipSetDevice(s.dev));
        const long ncell = (long)s.nyl * nx;
        hipLaunchKernelGGL(lbm::lbm_mean_add, dim3(cdiv(ncell, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc, s.lat[c->cur], s.plane, s.pitch,
                           nx, ncell, s.blocked, c->p.density, (float*)macc[i].p);
        HIPC(hipGetLastError());
      }
    if (ws && done % se == 0) {
      if ((rc = derive_all(c, what->fields_out + (size_t)jsnap * (size_t)slot, nullptr, nullptr, s_dev))) return rc;
      ++jsnap;
    }
  }
  // ---- the means, and what was staged for the host
  for (size_t i = 0; i < ns; ++i) {
    Slab& s = c->slabs[i];
    HIPC(hipSetDevice(s.dev));
    if (wm) {
      const long ncell = (long)s.nyl * nx;
      hipLaunchKernelGGL(lbm::lbm_mean_div, dim3(cdiv(ncell, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc, (const float*)macc[i].p, ncell,
                         (float)mm, mean_of(i));
      HIPC(hipGetLastError());
    }
    HIPC(hipStreamSynchronize(s.sc));
    if (wm && !m_dev)
      HIPC(hipMemcpy(what->mean_out + 4L * (s.row0 - base_row) * nx, macc[i].p, sizeof(float) * 4 * (size_t)s.nyl * (size_t)nx, hipMemcpyDeviceToHost));
  }
  if (wp && !p_dev) {
    std::vector<float> tmp;
    for (size_t i = 0; i < ns; ++i) {
      Slab& s = c->slabs[i];
      if (s.pcells_host.empty()) continue;
      HIPC(hipSetDevice(s.dev));
      if (s.pcells_host.size() == (size_t)np) {            // (every probe is this slab's)
        HIPC(hipMemcpy(what->probes_out, pstage[i].p, sizeof(float) * pfloat, hipMemcpyDeviceToHost));
        continue;
      }
      tmp.resize(pfloat);
      HIPC(hipMemcpy(tmp.data(), pstage[i].p, sizeof(float) * pfloat, hipMemcpyDeviceToHost));
      for (int j = 0; j < mp; ++j)
        for (const int4& q : s.pcells_host) {
          const size_t o = 4 * ((size_t)j * np + (size_t)q.z);
          memcpy(what->probes_out + o, tmp.data() + o, 4 * sizeof(float));
        }
    }
  }
  c->gpu_ms = gpu_ms; c->wall_ms = wall_ms;
  c->observed_in_kernel = bits; c->observed_in_wave = wbits; c->observed_pieces = pieces;
  return LBM_OK;
}
