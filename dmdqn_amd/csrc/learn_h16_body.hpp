// learn_h16_body.hpp -- the whole learn of one agent by its workgroup: the body
// of the learn kernels of learn_h16.hpp, included as text inside each of them
// (k_learn_*: once; k_learn_*_x2: the body of its two rounds).  As text and not
// as a __forceinline__ function: through a function the same statements reached
// the register allocator in another order and the float-row and soft-update
// instantiations gained 4-16 B of scratch per lane (tools/kernel_resources.py).
// The including scope provides: dmdqn_learn_args a (this scope's own copy:
// hp_apply overwrites it), float *gout, dmdqn_agent_hparams hp, and the
// compile-time flags QSTATS, TM, GOUT, XF, TS, HP (learn_h16.hpp describes them).
    LEARN_SMEM_SETUP;
    const int agent = blockIdx.x;
    if constexpr (HP) hp_apply(a, hp, agent);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lg = l >> 4;
    const size_t Pz = (size_t)L::P;
    float *Wp = a.params + agent * Pz, *Mp = a.adam_m + agent * Pz, *Vp = a.adam_v + agent * Pz;
    float *Tp = a.target + agent * Pz;
    const size_t Ph = (Pz + 7) / 8 * 8;
    h16 *TH = TS ? reinterpret_cast<h16 *>(a.target_h) + agent * Ph : nullptr;
    static_assert(TM != TGT_SOFT || (TS && !GOUT), "soft: with the shadow, fused learn only");
    const AdamC AK{a.alpha, a.c1, a.c2, a.eps, GOUT ? TGT_NONE : TM, TH, GOUT,
                   GOUT ? gout + agent * Pz : nullptr, a.tau, a.one_minus_tau};
    STAMP(0);
    // Issue order (vmcnt is in-order): the deque positions, the output layers,
    // then the target's fragments -- so the slot computation waits only for
    // the positions and the S' row gather goes out while the fragments land
    // (round 4 stored the output layers to LDS right after issuing the
    // fragments: the head then waited for every fragment before the gather)
    const int pos = batch_pos(a, agent);
    const OutStage so_on = stage_out_load(Wp);
    OutStage so_tg;
    if constexpr (TS) so_tg = stage_out_load(TH);
    else so_tg = stage_out_load(Tp);
    Frags fr;
    if constexpr (TS) load_frags(TH, fr);  // in flight during the z-score + gather
    else load_frags(Tp, fr);

    // ---- slots, X(S') + metadata from the s' rows, z-score (the output
    // layers' LDS images are synced by its barriers)
    batch_head<XF>(a, agent, pos, R2, S, [&]() {
        stage_out_store(so_on, W3L, B3L);
        stage_out_store(so_tg, W3L + NACT * H, B3L + NACT);
    });
    STAMP(1);
    STAMP(2);
    // ---- target(S') -> z3 ; online(S') -> Q ; y
    // target forward keeps X(S') in R2; the online net's fragments (reused by
    // both online forwards) load layer by layer as the target's die
    const float *Wpc = Wp;
    // Buffer plan: target X=R2 -> H1 R1 -> H2 R1 (hold; X survives) ;
    // online S': X=R2 -> H1 R1 -> H2 R2 over the dead X (no hold), the S rows
    // issued after layer 1 land in R1 once layer 2 is done ; training forward:
    // X=R1 -> H1 R2 -> H2 R1 over X (no hold).  The backward then finds H1 in R2
    // and H2 in R1: it runs on the swapped pair (P1, P2) = (R2, R1).
    forward_x<true>(fr, tg, R2, R1, R1, S.z3, [Wpc](Frags &f) { load_w1(Wpc, f); },
                    [Wpc](Frags &f) { load_w2(Wpc, f); });
    STAMP(3);
    float *qo = (float *)DQ;
    RowsT<XF> gs;
    forward_x<false>(fr, on, R2, R1, R2, qo,
                     [&](Frags &) { gather_x<XF>(a, agent, false, S.slot, gs); }, NoHook{},
                     [&]() { commit_x<XF>(R1, gs); });
    STAMP(4);
    STAMP(5);
    ddqn_target(a, qo, S);
    STAMP(6);
    forward_x<false>(fr, on, R1, R2, R1, S.z3);
    h16 *const P1 = R2, *const P2 = R1;
    STAMP(7);
    const half8 ones = ones8();
    loss_dq<QSTATS>(a, agent, DQ, S);
    // ---- dW3[k][a] = H2^T . DQ (wave w: k-tile w) ; db3 (wave 0)
    {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, gb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b0 = 0; b0 < B_; b0 += 32) {
            half8 dqf = frag_tr(DQ, 16, b0, 0);
            acc = mfma(frag_tr_h(P2, b0, 16 * w), dqf, acc);
            gb = mfma(ones, dqf, gb);  // every wave (no MFMA under divergent control)
        }
        if (lr < NACT) {
            // rows k = 16w + 4lg + e (consecutive), column a: W3T[a][k..k+3]
            adam4(Wp, Mp, Vp, Tp, L::oW3T + (size_t)lr * H + 16 * w + 4 * lg, acc, AK);
            if (w == 0 && lg == 0) adam1(Wp, Mp, Vp, Tp, L::ob3 + lr, gb[0], AK);
        }
    }
    __syncthreads();  // dW3 read H2; dZ2 overwrites it
    STAMP(8);
    bwd_dz2(P2, on, S);
    STAMP(9);
    h1_mask(P1, mask);  // the DQ region is free now
    // ---- dW2[j][k] = H1^T . dZ2 (wave w: j-tile w, 8 k-tiles) ; db2 (k-tile w) ; Adam
    {
        f32x4 g2[8], gb = {0.f, 0.f, 0.f, 0.f};
        // rows j = 16w + 4lg + e, column k = 16t + lr  ->  W2T[k][j..j+3]
        adam_pipe<4, 2, false>(
            Wp, Mp, Vp, Tp,
            [&](int t) { return (size_t)L::oW2T + qn_wt(16 * t + lr, 16 * w + 4 * lg, H); }, g2,
            AK, [&]() {
#pragma unroll
                for (int t = 0; t < 8; t++) g2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b0 = 0; b0 < B_; b0 += 32) {
                    const half8 av = frag_tr_h(P1, b0, 16 * w);
                    gb = mfma(ones, frag_tr_h(P2, b0, 16 * w), gb);
#pragma unroll
                    for (int t = 0; t < 8; t++) g2[t] = mfma(av, frag_tr_h(P2, b0, 16 * t), g2[t]);
                }
                // H1 fully consumed (dW2, mask): P1 becomes the W2^T image now,
                // from the register copy of old W2 (fr.w2), dead during Adam
                __syncthreads();
                w2t_image(P1, fr);
            });
        const int tx = fresh_tid();  // (16w + lr kept from the head spilled)
        if ((tx & 63) < 16) adam1(Wp, Mp, Vp, Tp, L::ob2 + (tx >> 6) * 16 + (tx & 15), gb[0], AK);
    }
    __syncthreads();  // W2^T image complete
    f32x4 d1[8];
    bwd_dh1_from_image(P1, P2, d1);
    {
        RowsT<XF> gx;  // X(S) again for dW1 (P2 is free)
        gather_x<XF>(a, agent, false, S.slot, gx);
        commit_x<XF>(P2, gx);
    }
    STAMP(10);
    bwd_dz1(P1, mask, d1);
    __syncthreads();
    STAMP(11);
    // ---- dW1[i][j] = X^T . dZ1 (wave w: j-tile w, 6 i-tiles) ; db1 (j-tile w)
    {
        const int tx = fresh_tid(), lr = tx & 15, lg = (tx & 63) >> 4;
        f32x4 g1[6], gb = {0.f, 0.f, 0.f, 0.f};
        // rows i = 16t + 4lg + e, column j = 16w + lr -> W1T[j][i..i+3]; tile 5
        // holds features 80..95: lanes lg < 2 (80..87) update in the pipe, lane
        // lg = 2's first row is feature 88 (the W1T column, below), the rest
        // (89..95) do not exist
        adam_pipe<2, 3, true>(
            Wp, Mp, Vp, Tp,
            [&](int t) { return (size_t)L::oW1T + qn_w1<H>(16 * w + lr, t < 5 || lg < 2 ? 16 * t + 4 * lg : 0); },
            g1, AK, [&]() {
#pragma unroll
                for (int t = 0; t < 6; t++) g1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b0 = 0; b0 < B_; b0 += 32) {
                    const half8 bv = frag_tr_h(P1, b0, 16 * w);
                    gb = mfma(ones, bv, gb);
#pragma unroll
                    for (int t = 0; t < 6; t++)
                        g1[t] = mfma(frag_tr_h<DP>(P2, b0, 16 * t), bv, g1[t]);
                }
            },
            [&](int t) { return t < 5 || lg < 2; });
        // b1[j] (lanes lg = 0: every row of the ones-MFMA holds the column sum)
        // and W1T[j][88] (lanes lg = 2, row 88 of tile 5)
        if (lg == 0 || lg == 2)
            adam1(Wp, Mp, Vp, Tp, (lg == 0 ? L::ob1 : L::oW1X) + 16 * w + lr,
                  lg == 0 ? gb[0] : g1[5][0], AK);
    }
    if (a.stamps) {
        __syncthreads();
        STAMP(12);
    }
