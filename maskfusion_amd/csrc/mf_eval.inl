// mf_eval.inl -- mf_model_cloud_nn_dev: the nearest-neighbour query against a model's live map, in place (kernels: mf_eval.hip).
// (part of mf_context.hip, included after the model list helpers)

// Scratch of the model query, allocated on the first call, grown on demand and freed by mf_destroy: nothing of it is shared with the frame path.
struct EvalScratch {
    int* d_offs = nullptr; size_t offs_cap = 0;          // run offsets + the live count
    int* h_total = nullptr;                              // pinned
    float4* d_pts = nullptr; size_t pts_cap = 0;         // the live surfels' positions in download order
    void* d_ws = nullptr; uint64_t ws_cap = 0;           // mf_cloud_nn_dev's workspace
    ~EvalScratch() {
        for (void* p : {(void*)d_offs, (void*)d_pts, d_ws})
            if (p) (void)hipFree(p);
        if (h_total) (void)hipHostFree(h_total);
    }
};
static void eval_free(EvalScratch* e) { delete e; }

extern "C" int mf_model_cloud_nn_dev(mf_ctx* c, int32_t model, float conf_threshold, const float* d_query, int32_t query_stride, int64_t n_query,
                                     const float* query_to_model16, float radius, float* d_dist, int32_t* d_idx) {
    settle(c);
    if (!c) return MF_EINVAL;
    ModelState* m = model_at(c, model);
    if (!m) { c->err = "mf_model_cloud_nn_dev: no such model"; return MF_EINVAL; }
    if (!(conf_threshold == conf_threshold)) { c->err = "mf_model_cloud_nn_dev: confidence threshold is NaN"; return MF_EINVAL; }
    int rc = mf_sync(c);   // (the object stream's work included: the buffers are read as the last frame left them)
    if (rc != MF_OK) return rc;
    if (!c->eval) c->eval = new EvalScratch();
    EvalScratch& e = *c->eval;
    hipStream_t s = c->stream;
    const size_t runs = run_table_runs((long)m->cap, (long)c->P) + 2;
    if (!e.h_total) MF_HIP(c, hipHostMalloc(&e.h_total, sizeof(int)));
    if (runs > e.offs_cap) {
        if (e.d_offs) MF_HIP(c, hipFree(e.d_offs));
        e.d_offs = nullptr; e.offs_cap = 0;
        MF_HIP(c, hipMalloc(&e.d_offs, runs * sizeof(int)));
        e.offs_cap = runs;
    }
    const Surfels& sf = m->surf[m->cur];
    launch_run_offsets(sf, m->d_frame, e.d_offs, e.d_offs + (runs - 1), s);
    MF_HIP(c, hipMemcpyAsync(e.h_total, e.d_offs + (runs - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    MF_HIP(c, hipStreamSynchronize(s));
    const int n = std::max(0, std::min(*e.h_total, m->cap));
    if ((size_t)n > e.pts_cap) {
        if (e.d_pts) MF_HIP(c, hipFree(e.d_pts));
        e.d_pts = nullptr; e.pts_cap = 0;
        MF_HIP(c, hipMalloc(&e.d_pts, (size_t)n * sizeof(float4)));
        e.pts_cap = (size_t)n;
    }
    const uint64_t need = nn_workspace_bytes(n);
    if (need > e.ws_cap) {
        if (e.d_ws) MF_HIP(c, hipFree(e.d_ws));
        e.d_ws = nullptr; e.ws_cap = 0;
        MF_HIP(c, hipMalloc(&e.d_ws, need));
        e.ws_cap = need;
    }
    if (n > 0) launch_nn_gather(sf, m->d_frame, e.d_offs, conf_threshold, e.d_pts, n, (int)(runs - 2), s);
    const char* why = nullptr;
    rc = nn_run((const float*)e.d_pts, 4, n, d_query, query_stride, n_query, query_to_model16, radius, d_dist, d_idx, e.d_ws, e.ws_cap, s, &why);
    if (rc != MF_OK) c->err = std::string("mf_model_cloud_nn_dev: ") + (why ? why : "failed");
    return rc;
}
