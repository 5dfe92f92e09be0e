// Host side of run_chain (bhg_mlp.hip), no device code: the mode a caller asks for, the plan derived from it before the first launch,
// and the state one stage leaves for a later one.  Included inside namespace bhg, after SolvePlan / FusedWs / SideState.

// What one pass of the HVP chain does with its weight-shaped outputs.
struct ChainMode {
  int mode;                     // FUSE_NONE: store H*dir into out[] | FUSE_CG | FUSE_NEUMANN
  void* const* out;             // FUSE_NONE
  float* fa; float* fb; float* fd;   // fused: flat bases of FuseArgs a / b / d
  const int64_t* starts;        // fused: element offsets of the 2L tensors inside the flat vectors
  float alpha, shift, out_scale;
  int apply_out;
  // FUSE_CG
  FusedWs* ws;
  const double* partRR_old; int nRR_old;
  const double* partPP; int nPP;
  double* partRR_new;
  double* scal;
  float cg_alpha;
  int kpar;                     // iteration parity
  int x_mode;                   // see FuseArgs.x_mode (applies to the lazy slices only)
  int first;                    // first iteration of a solve (Rz(x) accumulator is set, not added to)
  int lazy;                     // the direction at fd is the previous one; this iteration's is fa + beta * fd
  double* rzx_acc;              // FUSE_NEUMANN without an accumulator vector: sum_k Rz(v_k) lands here (head kernel)
  int skip_outputs;             // FUSE_CG: stop after the step length (see bhg_mlp_cg_solve)
  int gemm_mode;                // FUSE_NONE: BHG_MLP_WSK-style mode asked for by the caller (bhg_mlp_hvp_mode)
  const SolvePlan* sp;          // fused: the form of the whole solve (plan_solve decides; every pass of a solve is handed the same one)
  const BetaArgs* beta; int beta_blocks;   // hoisted form: k_cg_beta's work rides in k_hoist's launch (iterations > 0)
  int stop_after_head;          // projected Neumann: the closing pass that only adds Rz(v_K) to the accumulated Rz sums
  // global-batch CG (bhg_mlp_cg_global_phase): the iteration is cut where the ranks must talk.
  //   gphase 1: the R-chain only; this rank's share of p.H_data p -> php[0] (k_php_local)
  //   gphase 2: step length from the all-reduced php[0] * inv_world, then the outputs with their epilogues
  int gphase; double* php; double inv_world;
  int second;                   // fully projected CG: iteration 1 (the scalars k_proj_step completes are those of the FIRST iteration)
  int nk;                       // projected Neumann: iteration index (the row-major Rh_0 lives in two slots by its parity, see vnew)
  const void* const* rhs;       // fully projected CG, first iteration: the right-hand side's own tensors (bhg_mlp_cg_solve_rhs) or NULL
};

// What one pass of the chain decides before its first launch (plan_chain).  The stages of run_chain read it; none of them changes it.
struct ChainPlan {
  int L;
  float rho2;                   // ridge term of the stored outputs (FUSE_NONE; the fused recurrences carry theirs in `shift`)
  bool cg;                      // FUSE_CG
  bool no_fuse, no_outer_all;   // A/B switches (debug)
  bool single;                  // one stream, no events, all weight-shaped outputs in one launch after the chain
  bool no_side;                 // nothing runs on the side stream: `single`, or the A/B switch mlp_no_side
  bool head;                    // the narrow-head kernels apply (use_head)
  SideState* ss;                // the library-owned side stream and its events
  int tn, wsk;                  // skinny_tile_n(); form of the skinny GEMMs (wsk_mode)
  FuseArgs fbase;               // what the fused epilogues of every tensor share (fuse_at adds the tensor's slices)
  // r'.r' partial slots of the fused CG epilogues: [W_0 tiles][W_1 tiles]...[bias blocks]
  int part_base_w[BHG_MLP_MAX_LAYERS], part_base_bias;
  // the hoisted form (every direction product in ONE grouped launch, then the chain with the constant weights only), or NULL.
  // CG: needs the lazy direction (G(p) = G(r) + beta G(p_old)); Neumann: the direction v is explicit, G(v) directly
  const HoistPlan* hp;
  float* hoist;                 // hp: slabs + G arrays inside the fused workspace (FusedWs.hoist)
  float* rh0;                   // m->Rh[0]
  bool do_chain;                // (global-batch CG, second phase: the chain ran in the first)
  // projected CG, not the last iteration (projected Neumann: EVERY iteration): the iteration ends with the G(raw) products
  bool proj_iter;
  // the per-iteration Gram products T_l / E_l as extra workgroups of the chain launch that consumes the same packed activation
  // (debug key packed_gram: A/B); graw2: this pass closes with k_graw
  bool gram_in_chain, graw2;
  // Properties of the WHOLE solve, copied from SolvePlan (described there) for the stages to read; all zero where this pass runs the
  // classic chain.  proj: SolvePlan.proj_level
  int proj;
  bool packed, graw_single, rnew, vnew, lin, lin_head, head_j;

  float* rh0_slot(int k) const { return (k & 1) ? hoist + hp->rh0alt_off : rh0; }                   // Rh_0(v_k), row-major (vnew)
  float* gp1(int par) const { return hoist + (par ? hp->gp1alt_off : hp->g_off[hp->gf[1]]); }       // Gf_1(p): two slots (lin)
  float* gp2(int par) const { return hoist + (par ? hp->gp2alt_off : hp->g_off[hp->gf[L - 2]]); }   // Gf_{L-2}(p): two slots (lin_head)
  // Gram products riding in chain launches: ONE K slab each — every rider sits in a launch whose tiles have the same K (T_1 with
  // the forward product through W_1; E_l and T_{l+1} with the backward product through W_l), so it ends when they do
  // (read by the measurement build's G(raw) launch only)
  int gram_slabs(int K) const { return gram_in_chain ? 1 : gram_ksplit(K); }
};

// What one stage of run_chain leaves for a later one.
struct ChainState {
  HeadFuse head_fuse{};               // the pre-head product left raw K-split slabs: the head kernel combines them itself
  bool fuse_head = false;
  PstepArgs lin_ps{};                 // lin: the update blocks' arguments, built where k_pstep would be launched, used by the first product's launch
  int lin_nu = 0, lin_U = 4;
  bool lin_update_pending = false;    // the update blocks ride in the launch after the first product (k_wskpu) or in the head launch (k_headu)
  bool sd_in_chain = false;           // first iteration: S_l, D_l rode in the first chain launch as well
  bool head_j = false;                // this pass skipped the pre-head launch: the head launch is k_headj, T2h arrives as tile partials
  int head_j_nt = 0;                  // ... behind the layers' own in partT2 (0: in partT2h's slots)
  double* head_j_t2h = nullptr;       // ... or, 16 x 16 tiles, by pairs of tiles in this buffer of B slots, which the step length sums as partT2h
};

int plan_chain(const bhg_mlp* m, const ChainMode& cm, ChainPlan* p) {
  const int L = m->L;
  *p = ChainPlan{};
  p->L = L;
  p->rho2 = cm.mode == FUSE_NONE ? m->ridge2 : 0.f;
  const bool cg = p->cg = cm.mode == FUSE_CG;
  const bool no_side_env = dbg(DBG_mlp_no_side, 0) != 0;    // A/B switches (debug)
  p->no_fuse = dbg(DBG_mlp_no_fuse, 0) != 0;
  p->no_outer_all = dbg(DBG_mlp_no_outer_all, 0) != 0;
  const bool neumann_side = dbg(DBG_neumann_side, 0) != 0;    // A/B: fused Neumann with side-stream outputs
  p->single = cg || (cm.mode == FUSE_NEUMANN && !neumann_side && !p->no_outer_all);
  p->no_side = no_side_env || p->single;
  p->head = use_head(m);
  BHG_REQUIRE(!cg || p->head, "the fused CG solver needs the narrow-head kernels");
  if (int rc = side_state(&p->ss)) return rc;
  p->tn = skinny_tile_n();
  p->wsk = wsk_mode(cm.mode, cm.gemm_mode);

  FuseArgs& fbase = p->fbase;
  fbase.scal = cm.scal; fbase.part = cm.partRR_new; fbase.alpha = cm.alpha; fbase.shift = cm.shift;
  fbase.out_scale = cm.out_scale; fbase.apply_out = cm.apply_out;
  fbase.part_stride = cg ? cm.ws->nRR : 0;
  fbase.kpar = cm.kpar;
  int base = 0;
  for (int l = 0; l < L; ++l) { p->part_base_w[l] = base; base += outer_blocks(m, l, p->head); }
  p->part_base_bias = base;

  const SolvePlan* sp = cm.sp;
  const HoistPlan* hp = p->hp = (sp && sp->hoist && (cg || p->single)) ? &sp->hp : nullptr;
  p->hoist = hp ? cm.ws->hoist : nullptr;
  p->rh0 = m->Rh[0];
  p->do_chain = cm.gphase != 2;
  if (hp) { p->proj = sp->proj_level; p->packed = sp->packed; p->graw_single = sp->graw_single; p->rnew = sp->rnew; p->vnew = sp->vnew; }
  if (hp) { p->lin = sp->lin; p->lin_head = sp->lin_head; p->head_j = sp->head_j; }
  p->proj_iter = hp && p->proj && (cg ? (!cm.apply_out && !cm.skip_outputs) : true);
  p->gram_in_chain = p->packed && p->proj_iter && !cm.stop_after_head && dbg(DBG_packed_gram, 1) != 0;
  p->graw2 = p->gram_in_chain && p->graw_single;
  return BHG_OK;
}

// The fused epilogue's arguments for one of the 2L tensors.
FuseArgs fuse_at(const ChainMode& cm, const ChainPlan& pl, int tensor, int part_base) {
  FuseArgs f = pl.fbase;
  if (cm.mode != FUSE_NONE) {
    const int64_t o = cm.starts[tensor];
    f.a = cm.fa + o; f.b = cm.fb ? cm.fb + o : nullptr; f.d = cm.fd + o;
    // lazy direction: only the MFMA layers' weight slices (the small slices were updated by k_cg_beta)
    f.lazy = cm.lazy && (tensor & 1) == 0 && !(pl.head && tensor == 2 * (pl.L - 1));
    f.x_mode = (f.lazy || cm.mode == FUSE_NEUMANN) ? cm.x_mode : 0;
    if (!cm.fb) f.x_mode = 1;   // fused CG without a solution vector: nothing reads or writes x
  }
  f.part_base = part_base;
  return f;
}
