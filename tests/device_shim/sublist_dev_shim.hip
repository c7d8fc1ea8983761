// Device-compiled view of MsmSort::sublist (msm_driver_impl.cuh: k_msm_sub_mark, scan_u32, k_msm_sub_emit,
// k_msm_sub_starts) on a sorted entry list the CALLER supplies: tests/test_msm_sublist_gpu.py builds lists no digit sort would
// give it on demand - a bucket over three tiles, empty buckets on a tile boundary, lengths around a multiple of the tile -
// and compares the sub-list word for word with a filter of the source.  Test-only; never part of libhekaton.
//
// The shim checks what the kernels take on trust (start monotone and within n W, every index below n, every rank below
// n_dst, no more kept entries than the sub-list holds) and refuses anything else before a launch; it allocates and frees
// its own buffers, returns every HIP status, and never touches an hk_ctx.
#include "../../hekaton_system_amd/csrc/msm_driver_impl.cuh"
#include "shim_common.cuh"

extern "C" {
// plan words of the source plan (n scalars, window c, WP = 1, BN254 Fr) and the sub-list plan over n_dst of them:
// out[0..6] = W, NB, gshift_src, gshift_dst, sorted stride src, sorted stride dst, tiles per proof
int dshim_sublist_plan(unsigned c, unsigned n, unsigned n_dst, unsigned* out) {
    typedef CurveBn254::Fr Fr;
    if (c < 3 || c > 16 || n == 0 || n > (1u << 20) || n_dst == 0 || n_dst > n) return SHIM_REFUSED;
    MsmPlan ps = msm_make_plan(n, CurveBn254::FR_BITS, c, 1u, 262144u, Fr::Params::MOD, Fr::Params::N);
    MsmPlan pd = msm_sub_plan(ps, n_dst, 262144u);
    out[0] = ps.W; out[1] = ps.NB; out[2] = ps.gshift; out[3] = pd.gshift;
    out[4] = (unsigned)msm_sorted_stride(ps); out[5] = (unsigned)msm_sorted_stride(pd); out[6] = msm_sub_tiles(ps);
    return 0;
}

// sorted_src: batch slices of the source stride, start_src: batch x (NB + 1), rank: n words (MSM_RANK_NONE or < n_dst).
// sorted_dst / start_dst: batch slices of the sub-list's strides, as they lie before the call (the kernels write the kept
// entries and every start word, nothing else).  Returns 0, SHIM_REFUSED, the product's hk_status, or minus a hipError_t.
int dshim_msm_sublist(unsigned c, unsigned batch, unsigned n, unsigned n_dst, const unsigned* sorted_src,
                      const unsigned* start_src, const unsigned* rank, unsigned* sorted_dst, unsigned* start_dst) {
    typedef CurveBn254::Fr Fr;
    if (c < 3 || c > 16 || batch == 0 || batch > 8 || n == 0 || n > (1u << 20) || n_dst == 0 || n_dst > n || !sorted_src ||
        !start_src || !rank || !sorted_dst || !start_dst)
        return SHIM_REFUSED;
    const MsmPlan ps = msm_make_plan(n, CurveBn254::FR_BITS, c, 1u, 262144u, Fr::Params::MOD, Fr::Params::N);
    const MsmPlan pd = msm_sub_plan(ps, n_dst, 262144u);
    const size_t ss = msm_sorted_stride(ps), sd = msm_sorted_stride(pd), st = ps.NB + 1;
    for (unsigned i = 0; i < n; i++)
        if (rank[i] != MSM_RANK_NONE && rank[i] >= n_dst) return SHIM_REFUSED;
    for (unsigned b = 0; b < batch; b++) {
        const unsigned* s = start_src + b * st;
        if (s[0] != 0 || s[ps.NB] > (u64)ps.n * ps.W) return SHIM_REFUSED;
        for (unsigned k = 0; k < ps.NB; k++)
            if (s[k] > s[k + 1]) return SHIM_REFUSED;
        size_t kept = 0;
        for (unsigned k = 0; k < s[ps.NB]; k++) {
            unsigned e = sorted_src[b * ss + k], i = e & ((1u << ps.gshift) - 1u);
            if (i >= n || ((e & 0x7fffffffu) >> ps.gshift) >= ps.F) return SHIM_REFUSED;
            kept += rank[i] != MSM_RANK_NONE;
        }
        if (kept > (size_t)pd.n * pd.W) return SHIM_REFUSED;
    }
    SortBufs src = {}, dst = {};
    u32* rank_d = nullptr;
    auto carve = [&](Carve& cv) {
        src.sorted = cv.n<u32>(ss * batch);
        src.start = cv.n<u32>(st * batch);
        rank_d = cv.n<u32>(n);
        MsmSort<Fr>::alloc_sub(cv, ps, pd, &dst, batch);
    };
    Carve count;
    carve(count);
    DevBufs d;
    Carve real;
    SHIM_GET(&real.base, count.off + 256, nullptr);                // one block, 0xA5: no stage may rely on cleared scratch
    carve(real);
    SHIM_TRY(hipMemcpy(src.sorted, sorted_src, ss * batch * 4, hipMemcpyHostToDevice));
    SHIM_TRY(hipMemcpy(src.start, start_src, st * batch * 4, hipMemcpyHostToDevice));
    SHIM_TRY(hipMemcpy(rank_d, rank, (size_t)n * 4, hipMemcpyHostToDevice));
    SHIM_TRY(hipMemcpy(dst.sorted, sorted_dst, sd * batch * 4, hipMemcpyHostToDevice));
    SHIM_TRY(hipMemcpy(dst.start, start_dst, st * batch * 4, hipMemcpyHostToDevice));
    hk_status hs = MsmSort<Fr>::sublist(0, ps, src, pd, rank_d, dst, batch);
    SHIM_TRY(hipDeviceSynchronize());
    if (hs != HK_OK) return (int)hs;
    SHIM_TRY(hipMemcpy(sorted_dst, dst.sorted, sd * batch * 4, hipMemcpyDeviceToHost));
    SHIM_TRY(hipMemcpy(start_dst, dst.start, st * batch * 4, hipMemcpyDeviceToHost));
    return 0;
}
}
