// body of k_msm_reduce_fused and its batched twin (msm.cuh, msm_batch.cuh): one source, so the single-proof kernel's code is unchanged
    __shared__ XYZZ<F> sh[MSM_REDUCE_THREADS];
    __shared__ u32 last;
    u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    u32 J = p.B / p.K;
    XYZZ<F> tot = XYZZ<F>::inf();
    if (t < J) {
        const XYZZ<F>* bk = buckets + (size_t)t * p.K;
        const u32* st = start + (size_t)t * p.K;
        XYZZ<F> run = XYZZ<F>::inf();
        for (int b = (int)p.K - 1; b >= 0; b--) {
            XYZZ<F> q = st[b] == st[b + 1] ? XYZZ<F>::inf() : ld_vec(&bk[b]);      // empty bucket: never written
            run = ec_add_ni(run, q);
            tot = ec_add_ni(tot, run);
        }
        u32 wgt = t * p.K;
        if (wgt && !run.is_inf()) {
            XYZZ<F> acc = XYZZ<F>::inf();
            for (int bit = 31 - __clz(wgt); bit >= 0; bit--) {
                acc = ec_dbl_ni(acc);
                if ((wgt >> bit) & 1) acc = ec_add_ni(acc, run);
            }
            tot = ec_add_ni(tot, acc);
        }
    }
    sh[threadIdx.x] = tot;
    __syncthreads();
    for (u32 off = MSM_REDUCE_THREADS / 2; off >= 1; off >>= 1) {
        if (threadIdx.x < off) {
            // operands stay in LDS (the out-of-line add takes references): two private copies of 384 B each less per
            // lane for the 12-limb G2 flavour, i.e. a smaller scratch ring on every queue that runs this kernel
            XYZZ<F> t = ec_add_ni(sh[threadIdx.x], sh[threadIdx.x + off]);
            sh[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st_vec(&partial[blockIdx.x], sh[0]);
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    XYZZ<F> acc = XYZZ<F>::inf();
    for (u32 j = threadIdx.x; j < gridDim.x; j += MSM_REDUCE_THREADS) acc = ec_add_ni(acc, ld_vec(&partial[j]));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (u32 off = MSM_REDUCE_THREADS / 2; off >= 1; off >>= 1) {
        if (threadIdx.x < off) {
            // operands stay in LDS (the out-of-line add takes references): two private copies of 384 B each less per
            // lane for the 12-limb G2 flavour, i.e. a smaller scratch ring on every queue that runs this kernel
            XYZZ<F> t = ec_add_ni(sh[threadIdx.x], sh[threadIdx.x + off]);
            sh[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) st_vec(res, sh[0]);
