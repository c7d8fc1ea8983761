// body of k_msm_accum0 and its batched twin (msm.cuh, msm_batch.cuh): one source, so the single-proof kernel's code is unchanged
    u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    u32 E = start[p.NB];
    LevelInfo li = msm_level_info(p, E, 0);
    // No memset precedes this launch.  The reduction's ticket (one u32 behind the buckets) is cleared here; a bucket with
    // no entries is never read (the reductions see start[b] == start[b + 1]); every other bucket is written exactly once by
    // the lane in whose slice it STARTS - its sum when it also ends there, the neutral element when it continues into the
    // next slices, whose partial sums the level kernels then add to it.
    if (t == 0) *reinterpret_cast<u32*>(buckets + p.NB) = 0u;
    if (t >= li.active) return;
    u32 pos = t * li.L;
    u32 end = min(pos + li.L, E);
    u32 b = msm_find_bucket(start, p.NB, pos);
    bool head_partial = start[b] < pos;
    bool first = true;
    u32 first_key = b;
    u32 boundary = start[b + 1];
    XYZZ<F> acc = XYZZ<F>::inf();
    // boundary partials go straight to memory when they become known (keeping a second XYZZ value
    // live across the loop costs 32+ VGPRs, i.e. a wave of occupancy)
    st_vec(&ppts[2 * t], XYZZ<F>::inf());
    if constexpr (AccumPrefetch<F>::value) {
        // software pipeline, two deep: the entry of step pos + 2 and the 64-byte table row of step pos + 1 are
        // requested before the mixed add of step pos, so neither link of the dependent chain entry -> row -> add
        // stands between two adds of this wave
        u32 e_n = 0, e_nn = 0;
        bool v_n = false;
        Affine<F> P_n;
        auto request_row = [&](u32 e) {
            e_n = e;
            u32 g = (e & 0x7fffffffu) >> p.gshift;
            u32 i = e & ((1u << p.gshift) - 1u);
            v_n = i >= idx_off && i - idx_off < n_bases;
            if (v_n) P_n = ld_vec(&bases[(size_t)g * n_bases + (i - idx_off)]);     // never touches an empty table
        };
        if (pos < end) request_row(sorted[pos]);
        if (pos + 1 < end) e_nn = sorted[pos + 1];
        for (; pos < end; pos++) {
            Affine<F> P = P_n;
            u32 e = e_n;
            bool v = v_n;
            if (pos + 1 < end) request_row(e_nn);
            if (pos + 2 < end) e_nn = sorted[pos + 2];
            if (pos == boundary) {
                if (first && head_partial) st_vec(&ppts[2 * t], acc);
                else st_vec(&buckets[b], acc);
                first = false;
                acc = XYZZ<F>::inf();
                do { b++; boundary = start[b + 1]; } while (boundary <= pos);
            }
            if (v) {
                if (e >> 31) P.y = F::neg(P.y);
                acc = ec_madd<F, AccumInlineCorner<F>::value>(acc, P);
            }
        }
    } else
    for (; pos < end; pos++) {
        if (pos == boundary) {
            // bucket b ended exactly here
            if (first && head_partial) st_vec(&ppts[2 * t], acc);
            else st_vec(&buckets[b], acc);
            first = false;
            acc = XYZZ<F>::inf();
            do { b++; boundary = start[b + 1]; } while (boundary <= pos);
        }
        u32 e = sorted[pos];
        u32 g = (e & 0x7fffffffu) >> p.gshift;
        u32 i = e & ((1u << p.gshift) - 1u);
        if (i >= idx_off && i - idx_off < n_bases) {
            Affine<F> P = ld_vec(&bases[(size_t)g * n_bases + (i - idx_off)]);
            if (e >> 31) P.y = F::neg(P.y);
            acc = ec_madd<F, AccumInlineCorner<F>::value>(acc, P);
        }
    }
    bool tail_partial = end < boundary;     // bucket b continues in the next lane's slice
    bool is_tail = false;
    if (first && head_partial) st_vec(&ppts[2 * t], acc);          // single run that began before this slice
    else if (tail_partial) { is_tail = true; st_vec(&buckets[b], XYZZ<F>::inf()); }   // starts here, continues: neutral
    else st_vec(&buckets[b], acc);
    pkeys[2 * t] = first_key;
    pkeys[2 * t + 1] = b;
    st_vec(&ppts[2 * t + 1], is_tail ? acc : XYZZ<F>::inf());
