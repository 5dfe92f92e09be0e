// The form a fused CG / Neumann solve takes, decided ONCE before its first launch (host only, no device code).  plan_solve is a pure
// function of the descriptor, its three arguments and the debug table: no device pointer, no workspace, no stream, no static state.
// The solvers (CgCtx, bhg_mlp_neumann_solve), every pass of the chain (ChainMode.sp, plan_chain), bhg_mlp_cg_state_mask and
// bhg_mlp_plan_describe all read THIS; none of them decides.  Included inside namespace bhg, after HoistPlan / headj_shape_ok.

// The descriptor checks the entry points share: a layer count the tables hold and a padded batch (tiled: of whole 128-row tiles)
inline bool mlp_desc_ok(const bhg_mlp* m) { return m && m->L >= 1 && m->L <= BHG_MLP_MAX_LAYERS && m->Bp > 0; }
inline bool mlp_desc_tiled(const bhg_mlp* m) { return mlp_desc_ok(m) && m->Bp % kTM == 0; }

struct SolvePlan {
  bool fused;                   // bhg_mlp_supports_fused_solve; false: nothing below is set (closing = k_outer_all), the callers run HVP + recurrence kernel
  HoistPlan hp;                 // computed once; ok = false where the solve does not ask for the hoisted forms
  bool lazy;                    // CG: the direction is r + beta * p_old, formed where it is read (k_cg_beta) | eager: the k_cg_pdir pass (A/B)
  bool hoist;                   // every direction product in one grouped launch (k_hoist), the chain through the constant weights only
  // CG: 1 = G(r) by recurrence, the N-sized r / p still updated by k_outer_all (the caller wants x); 2 = fully projected (default
  // without a solution vector): no N-sized state after the first iteration.  Neumann: 1 = projected (no accumulator vector).
  // (key mlp_proj: 0 off | 1 default | 9 level 1 even without a solution vector — the A/B arm of level 2)
  int proj_level;
  // packed: the chain through the constant weights on PACKED operands (wskp.inc; pack_operands, once per solve; key packed_chain: A/B)
  // graw_single: the iterations close with k_graw — what the NEXT iteration's recurrences are told about the layout of G(raw): one slab
  // per product, not one per pair (graw_single_on)
  bool packed, graw_single;
  // rnew (CG): k_graw computes the step length in its own launch and applies r' = r - alpha Hp to G(r) itself (GrawArgs.rnew): the next
  // iteration finds G(r) up to date, there is no G(raw)
  // vnew (Neumann): k_graw applies v' = v - alpha (raw + shift v) to G(v) itself and leaves Rh_0(v') packed and row-major — neumann.py:63
  // has no scalars to wait for — so the update launch at the top of the next iteration is gone: SIX launches instead of seven.  The
  // row-major Rh_0 alternates between m->Rh[0] and a second slot (iteration parity): the Gb_1 tiles that write Rh_0(v') still read Rh_0(v)
  bool rnew, vnew;
  int nt;                       // small tensors of the recurrences (BetaArgs.nt): L biases + the narrow head weight
  // lin: the chain's first product by linearity with the update launch riding in it (k_wskpl, wskpl.inc): every iteration's first product,
  // every k_graw (Rh_0(r') for the next one) and cg_iteration (the second bias's direction in slots) follow it | lin_head: on a four-layer
  // net the update blocks ride in the HEAD launch (k_headu), the pre-head launch is the plain product | head_j: ... whose rows read the
  // pre-head product through J (k_headj): no pre-head launch, its tiles ride in the head launch of every iteration but the first |
  // upd_first: deeper than four layers, the update blocks stay in k_wskpl behind the publisher of beta
  bool lin, lin_head, head_j, upd_first;
  int head_j_tile;              // head_j: the shape of the pre-head tiles in the head launch (head_j_tile(): 1 = 32 x 16, 2 = 16 x 16); else -1
  const char* closing;          // the launch that closes a projected iteration: k_outer_all | k_graw | k_grawk | k_hoist+k_proj_update
};

// algo 0: cg, 1: neumann.  keep_solution: the caller wants the N-sized x (cg) / accumulator p (neumann).  global: the global-batch CG
// solver (bhg_mlp_cg_global_phase) — lazy direction, N-sized residual (it is what the ranks exchange).
// Two facts the solvers used to read from workspace pointers are shape facts: carve_fused_ws carves Wf[1] iff hoist_plan(m).ok (which
// implies L >= 3), so "the packed operands exist" is hp.ok; and it sets nT2j > 0 iff headj_shape_ok(m, hp).
void plan_solve(const bhg_mlp* m, int algo, bool keep_solution, bool global, SolvePlan* sp) {
  memset(sp, 0, sizeof(*sp));
  sp->closing = "k_outer_all";
  sp->head_j_tile = -1;
  sp->fused = bhg_mlp_supports_fused_solve(m) != 0;
  if (!sp->fused) return;
  HoistPlan& hp = sp->hp;
  const bool head = use_head(m);
  sp->nt = m->L + (head ? 1 : 0);
  if (algo == 0) {
    // Direction update between two iterations: lazy (default; see k_cg_beta) or the 12*N-byte k_cg_pdir pass (A/B switch)
    sp->lazy = global || dbg(DBG_cg_eager_p, 0) == 0;
    if (sp->lazy && hoist_mode() != 0) hoist_plan(m, &hp);
    sp->hoist = sp->lazy && hp.ok;
    sp->proj_level = (!sp->hoist || !hp.proj_ok || proj_mode() == 0 || global) ? 0 : ((proj_mode() == 9 || keep_solution) ? 1 : 2);
  } else {
    // Hoisting alone (direction products on the N-sized v every iteration, mlp_hoist = 2) neither gains nor loses for Neumann (656 vs
    // 656 steps/s at cfg 2: no step length, no lazy direction, no beta launch to save) and is an A/B arm only; the projected form is
    // the default without an accumulator vector (whether K > 0 stays with the solve)
    const bool want_proj = !keep_solution && proj_mode() != 0 && hoist_mode() != 0;
    if (hoist_mode() == 2 || want_proj) hoist_plan(m, &hp);
    sp->hoist = hp.ok;
    sp->proj_level = (want_proj && hp.ok && hp.proj_ok && head) ? 1 : 0;
  }
  sp->packed = hp.ok && dbg(DBG_packed_chain, 1) != 0;
  sp->graw_single = graw_single_on(sp->packed, m->Bp);
  sp->rnew = algo == 0 && sp->graw_single && sp->proj_level >= 2 && rnew_keys_on();
  sp->vnew = algo == 1 && sp->proj_level && sp->graw_single && m->L >= 3 && dbg(DBG_neumann_vnew, 1) != 0;
  // lin: fully projected CG closing with the k_graw that applies the residual step, a net with a product between the first and the
  // pre-head one, few small tensors
  sp->lin = algo == 0 && sp->proj_level == 2 && hp.lin_ok && sp->rnew && sp->nt <= 16 && proj_step_merged() && dbg(DBG_pstep_v2, 1) != 0 &&
            dbg(DBG_lin_first, 1) != 0;
  // lin_head: the head's prefetching instance must apply (<= 12 classes, last hidden width <= 512); like lin it holds for the whole
  // solve (slot parity)
  sp->lin_head = sp->lin && m->L == 4 && dbg(DBG_lin_update_next, 1) != 0 && dbg(DBG_lin_update_in_head, 1) != 0 && dbg(DBG_lin_nub, 0) == 0 &&
                 m->dims[m->L] <= 12 && m->dims[m->L - 1] <= 512 && dbg(DBG_head_no_prefetch, 0) == 0;
  // head_j: J = W_3 diag(mask_2) W_2 is built once per solve, the pre-head launch leaves the dependency chain (bhg_mlp_headj.hip)
  sp->head_j = sp->lin_head && headj_shape_ok(m, hp) && dbg(DBG_head_j, 1) != 0;
  sp->head_j_tile = sp->head_j ? head_j_tile(m) : -1;
  sp->upd_first = sp->lin && m->L > 4;
  if (sp->proj_level >= 1) sp->closing = graw_batch_ok(m->Bp) ? (m->Bp == 128 ? "k_graw" : "k_grawk") : "k_hoist+k_proj_update";
}
