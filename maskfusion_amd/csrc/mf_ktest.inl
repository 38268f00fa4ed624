// mf_ktest.inl -- kernel-level entry points (mf_k_*: one reference CUDA wrapper or GLSL pass each) for the parity tests.
// (part of mf_context.hip: the library's host side is ONE translation unit -- the context type and its helpers are file-local -- kept in
// four files by subject; mf_context.hip includes them in this order)

// ------------------------------------------------------------------------------------------------
// kernel-level entry points
// ------------------------------------------------------------------------------------------------
static int launch_rc() { return hipGetLastError() == hipSuccess ? MF_OK : MF_EHIP; }

extern "C" int mf_k_bilateral(const float* d_depth, float* d_out, int32_t W, int32_t H, void* stream) {
    if (!d_depth || !d_out || W <= 0 || H <= 0) return MF_EINVAL;
    launch_bilateral(d_depth, d_out, W, H, (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_k_pyrdown_f(const float* d_src, float* d_dst, int32_t sw, int32_t sh, void* stream) {
    if (!d_src || !d_dst || sw < 2 || sh < 2) return MF_EINVAL;
    launch_pyrdown_f(d_src, d_dst, sw, sh, (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_k_intensity(const uint8_t* d_img, int32_t channels, uint8_t* d_out, int32_t n, void* stream) {
    if (!d_img || !d_out || n <= 0 || (channels != 3 && channels != 4)) return MF_EINVAL;
    launch_intensity(d_img, channels, d_out, n, (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_k_pyrdown_u8(const uint8_t* d_src, uint8_t* d_dst, int32_t sw, int32_t sh, void* stream) {
    if (!d_src || !d_dst || sw < 2 || sh < 2) return MF_EINVAL;
    launch_pyrdown_u8(d_src, d_dst, sw, sh, (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_k_derivative_images(const uint8_t* d_src, int16_t* d_dx, int16_t* d_dy, int32_t W, int32_t H, void* stream) {
    if (!d_src || !d_dx || !d_dy || W <= 0 || H <= 0) return MF_EINVAL;
    launch_derivative(d_src, d_dx, d_dy, W, H, 0.f, nullptr, (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_k_so3_prealign(const uint8_t* d_last, const uint8_t* d_next, int32_t W, int32_t H, float fx, float fy, float cx, float cy,
                                 double* R9, float* stats3, void* stream) {
    if (!d_last || !d_next || !R9 || !stats3 || W < 3 || H < 3) return MF_EINVAL;
    char* buf = nullptr;
    const size_t sb = so3_scratch_bytes(W, H);
    if (hipMalloc((void**)&buf, sb + sizeof(So3Result)) != hipSuccess) return MF_ENOMEM;
    So3Result* d = reinterpret_cast<So3Result*>(buf);
    if (launch_so3_prealign(d_last, d_next, W, H, Intr{fx, fy, cx, cy}, d, buf + sizeof(So3Result), (hipStream_t)stream) != 0) {
        (void)hipFree(buf);
        return MF_EINVAL;
    }
    So3Result h;
    (void)hipStreamSynchronize((hipStream_t)stream);
    const hipError_t e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return MF_EHIP;
    memcpy(R9, h.R, sizeof(h.R));
    stats3[0] = h.error; stats3[1] = h.count; stats3[2] = (float)h.iterations;
    return MF_OK;
}
static RgbLevel make_level(const int16_t* dIdx, const int16_t* dIdy, const float* lastDepth, const float* nextDepth, const uint8_t* lastImage,
                           const uint8_t* nextImage, int W, int H, float minScale, float maxDepthDelta) {
    RgbLevel L;
    L.dIdx = dIdx; L.dIdy = dIdy; L.lastDepth = lastDepth; L.nextDepth = nextDepth; L.lastImage = lastImage; L.nextImage = nextImage;
    L.W = W; L.H = H; L.minScale = minScale; L.maxDepthDelta = maxDepthDelta; L.gate = nullptr;
    return L;
}
extern "C" int mf_k_rgb_residual_gated(float min_scale, const int16_t* d_dIdx, const int16_t* d_dIdy, const float* d_last_depth,
                                       const float* d_next_depth, const uint8_t* d_last_image, const uint8_t* d_next_image, float max_depth_delta,
                                       const float* kt3, const float* krkinv9, int32_t W, int32_t H, void* d_corres, int32_t* count_sigma2,
                                       const uint8_t* d_gate_or_null, void* stream) {
    if (!d_dIdx || !d_dIdy || !d_last_depth || !d_next_depth || !d_last_image || !d_next_image || !kt3 || !krkinv9 || !d_corres ||
        !count_sigma2)
        return MF_EINVAL;
    float h[12];
    memcpy(h, krkinv9, 36); memcpy(h + 9, kt3, 12);
    char* scratch = nullptr;
    if (hipMalloc((void**)&scratch, 64) != hipSuccess) return MF_ENOMEM;
    float* d_k = reinterpret_cast<float*>(scratch);
    int* d_sums = reinterpret_cast<int*>(scratch + 48);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(d_k, h, 48, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_sums, 0, 8, s);
    if (e == hipSuccess) {
        RgbLevel L = make_level(d_dIdx, d_dIdy, d_last_depth, d_next_depth, d_last_image, d_next_image, W, H, min_scale, max_depth_delta);
        L.gate = d_gate_or_null;   // the branch production takes: the pose-independent tests read from the frame's gate image
        launch_rgb_residual_only(L, d_k, reinterpret_cast<RgbCorr*>(d_corres), d_sums, s);
        e = hipMemcpyAsync(count_sigma2, d_sums, 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    return e == hipSuccess ? MF_OK : MF_EHIP;
}
extern "C" int mf_k_rgb_residual(float min_scale, const int16_t* d_dIdx, const int16_t* d_dIdy, const float* d_last_depth,
                                 const float* d_next_depth, const uint8_t* d_last_image, const uint8_t* d_next_image, float max_depth_delta,
                                 const float* kt3, const float* krkinv9, int32_t W, int32_t H, void* d_corres, int32_t* count_sigma2,
                                 void* stream) {
    return mf_k_rgb_residual_gated(min_scale, d_dIdx, d_dIdy, d_last_depth, d_next_depth, d_last_image, d_next_image, max_depth_delta, kt3, krkinv9,
                                   W, H, d_corres, count_sigma2, nullptr, stream);
}
extern "C" int mf_k_rgb_step(const void* d_corres, float sigma, const float* d_last_depth, float fx, float fy, float cx, float cy,
                             const int16_t* d_dIdx, const int16_t* d_dIdy, float sobel_scale, int32_t W, int32_t H, double* out32,
                             void* stream) {
    if (!d_corres || !d_last_depth || !d_dIdx || !d_dIdy || !out32) return MF_EINVAL;
    double* d_out = nullptr;
    if (hipMalloc((void**)&d_out, 32 * sizeof(double)) != hipSuccess) return MF_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_out, 0, 32 * sizeof(double), s);
    if (e == hipSuccess) {
        launch_rgb_step_only(make_level(d_dIdx, d_dIdy, d_last_depth, d_last_depth, nullptr, nullptr, W, H, 0.f, 0.f),
                             reinterpret_cast<const RgbCorr*>(d_corres), sigma, Intr{fx, fy, cx, cy}, sobel_scale, d_out, s);
        e = hipMemcpyAsync(out32, d_out, 32 * sizeof(double), hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_out);
    return e == hipSuccess ? MF_OK : MF_EHIP;
}
extern "C" int mf_k_vmap_nmap(const float* d_depth, float* d_vmap, float* d_nmap, int32_t W, int32_t H, float fx, float fy, float cx,
                              float cy, float depth_cutoff, void* stream) {
    if (!d_depth || !d_vmap || !d_nmap || W <= 0 || H <= 0) return MF_EINVAL;
    launch_vmap_nmap(d_depth, d_vmap, d_nmap, W, H, Intr{fx, fy, cx, cy}, depth_cutoff, (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_k_model_pyramid(const float* d_v4, const float* d_n4, const float* R9, const float* t3, float* d_vmaps,
                                  float* d_nmaps, int32_t W, int32_t H, void* stream) {
    if (!d_v4 || !d_n4 || !R9 || !t3 || !d_vmaps || !d_nmaps || W % 4 || H % 4) return MF_EINVAL;
    float Rt[12];
    memcpy(Rt, R9, 36); memcpy(Rt + 9, t3, 12);
    float* vm[3]; float* nm[3];
    size_t off = 0;
    for (int i = 0; i < 3; ++i) {
        vm[i] = d_vmaps + off; nm[i] = d_nmaps + off;
        off += (size_t)(W >> i) * (H >> i) * 3;
    }
    launch_model_pyramid((const float4*)d_v4, (const float4*)d_n4, nullptr, nullptr, nullptr, Rt, vm, nm, W, H, Intr{1, 1, 0, 0},
                         (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_k_geometric_edges(const float* d_vmap, const float* d_nmap, float* d_edge, uint8_t* d_binary, uint8_t* d_tmp, int32_t W,
                                    int32_t H, float w_distance, float w_convexity, float threshold, int32_t morph_radius,
                                    int32_t morph_iterations, void* stream) {
    if (!d_vmap || !d_nmap || !d_edge || !d_binary || !d_tmp || W <= 2 || H <= 2) return MF_EINVAL;
    launch_edge_map(d_vmap, d_nmap, d_edge, W, H, w_distance, w_convexity, (hipStream_t)stream);
    launch_edge_binary(d_edge, d_binary, d_tmp, W, H, threshold, morph_radius, morph_iterations, (hipStream_t)stream);
    return launch_rc();
}
extern "C" int mf_segmentation_labels(int32_t W, int32_t H, const uint8_t* binary, const float* depth, const uint8_t* mask,
                                      const int32_t* class_ids, int32_t n_masks, const uint8_t* projected_ids, const int32_t* model_ids,
                                      const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new,
                                      const float* p, uint8_t* ignore_map, uint8_t* full, int32_t* has_new, int32_t* new_class) {
    if (!binary || !depth || !projected_ids || !model_ids || !model_class_ids || n_models < 1 || !p || !ignore_map || !full || !has_new ||
        !new_class || W <= 2 || H <= 2 || (n_masks > 0 && (!mask || !class_ids)))
        return MF_EINVAL;
    SegParams prm;
    prm.threshold = p[0]; prm.weightDistance = p[1]; prm.weightConvexity = p[2];
    prm.morphEdgeIterations = (int)p[3]; prm.morphEdgeRadius = (int)p[4]; prm.morphMaskIterations = (int)p[5]; prm.morphMaskRadius = (int)p[6];
    prm.removeEdges = p[7] != 0.f; prm.minRelSizeNew = p[8]; prm.maxRelSizeNew = p[9]; prm.personClassID = (int)p[10];
    std::vector<SegModelInfo> infos;
    for (int i = 0; i < n_models; ++i) infos.push_back(SegModelInfo{model_ids[i], model_class_ids[i]});
    std::vector<uint8_t> ign(ignore_map, ignore_map + (size_t)W * H);
    SegResult res;
    static const int32_t kNoClass[1] = {0};
    segmentation_host(prm, W, H, binary, depth, mask, n_masks > 0 ? class_ids : kNoClass, n_masks, projected_ids, infos, next_model_id,
                      allow_new != 0, ign, full, res);
    memcpy(ignore_map, ign.data(), ign.size());
    *has_new = res.hasNewLabel ? 1 : 0;
    *new_class = res.newClassID;
    return MF_OK;
}

// Device twin of mf_segmentation_labels (same arguments, HOST pointers; the images are staged to the device, the stage runs
// in mf_labels_gpu.hip, the outputs come back) -- the parity tests run both against the oracle.  mf_k_label_stage is the same
// call with the stage's intermediates readable and the jump rule's `alive` flags settable: one body serves both.
static __global__ void k_set_alive(PoseDev* p, int n) { if (blockIdx.x == 0 && (int)threadIdx.x < n) p[threadIdx.x].alive = threadIdx.x; }
extern "C" int mf_k_label_stage(int32_t W, int32_t H, const uint8_t* binary, const float* depth, const uint8_t* mask,
                                const int32_t* class_ids, int32_t n_masks, const uint8_t* projected_ids, const int32_t* model_ids,
                                const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new,
                                const float* p, uint8_t* ignore_map, uint8_t* full, int32_t* has_new, int32_t* new_class,
                                const int32_t* alive, int32_t* lab_cc, int32_t* lab_swept, int32_t* stats5, int32_t* n_comp,
                                int32_t stats_cap) {
    if (!binary || !depth || !projected_ids || !model_ids || !model_class_ids || n_models < 1 || n_models > 64 || !p || !ignore_map ||
        !full || !has_new || !new_class || W <= 2 || H <= 2 || (n_masks > 0 && (!mask || !class_ids)) || n_masks > 256 ||
        (stats5 && stats_cap < 0))
        return MF_EINVAL;
    SegParams prm;
    prm.threshold = p[0]; prm.weightDistance = p[1]; prm.weightConvexity = p[2];
    prm.morphEdgeIterations = (int)p[3]; prm.morphEdgeRadius = (int)p[4]; prm.morphMaskIterations = (int)p[5]; prm.morphMaskRadius = (int)p[6];
    prm.removeEdges = p[7] != 0.f; prm.minRelSizeNew = p[8]; prm.maxRelSizeNew = p[9]; prm.personClassID = (int)p[10];
    const size_t P = (size_t)W * H;
    LabelsScratch sc;
    if (!sc.init((int)P)) return MF_ENOMEM;
    uint8_t *d_bin = nullptr, *d_mask = nullptr, *d_proj = nullptr, *d_full = nullptr; float* d_depth = nullptr; PoseDev* d_pose = nullptr;
    if (!sc.dalloc(&d_bin, P) || !sc.dalloc(&d_mask, P) || !sc.dalloc(&d_proj, P) || !sc.dalloc(&d_full, P) || !sc.dalloc(&d_depth, P) ||
        !sc.dalloc(&d_pose, 2))
        return MF_ENOMEM;
    hipStream_t s = nullptr;
    hipError_t e = hipMemcpy(d_bin, binary, P, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_proj, projected_ids, P, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_depth, depth, P * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_masks > 0) e = hipMemcpy(d_mask, mask, P, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(sc.ignoreMap, ignore_map, P, hipMemcpyHostToDevice);
    if (e != hipSuccess) return MF_EHIP;
    hipLaunchKernelGGL(k_set_alive, dim3(1), dim3(64), 0, s, d_pose, 2);   // one pose per distinct flag value: [0] dropped, [1] alive
    std::vector<SegModelInfo> infos;
    std::vector<const PoseDev*> poses;
    for (int i = 0; i < n_models; ++i) {
        infos.push_back(SegModelInfo{model_ids[i], model_class_ids[i]});
        poses.push_back(d_pose + ((alive && i > 0 && alive[i] == 0) ? 0 : 1));
    }
    static const int32_t kNoClass[1] = {0};
    int rc = sc.enqueue(prm, W, H, d_bin, d_depth, n_masks > 0 ? d_mask : nullptr, n_masks > 0 ? class_ids : kNoClass, n_masks, d_proj, infos,
                        poses, next_model_id, allow_new != 0, d_full, s);
    if (rc != MF_OK) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return MF_EHIP;
    // the component half ran before the vote tables were sized: readable whether or not they fit
    const int nc = sc.h_result[3];
    if (n_comp) *n_comp = nc;
    if (lab_cc && hipMemcpy(lab_cc, sc.lab[0], P * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return MF_EHIP;
    if (lab_swept && hipMemcpy(lab_swept, sc.lab[prm.removeEdges ? 1 : 0], P * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return MF_EHIP;
    if (stats5) {   // cv::connectedComponentsWithStats order: left, top, width, height, area; row 0 (the background, never read by the stage) is not written
        const int rows = std::min(nc, (int)stats_cap);
        std::vector<int32_t> h_area((size_t)std::max(rows, 1));
        std::vector<int4> h_box((size_t)std::max(rows, 1));
        if (rows > 0 && (hipMemcpy(h_area.data(), sc.area, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(h_box.data(), sc.bbox, (size_t)rows * sizeof(int4), hipMemcpyDeviceToHost) != hipSuccess))
            return MF_EHIP;
        for (int c = 1; c < rows; ++c) {
            const int4 b = h_box[c];
            stats5[c * 5 + 0] = b.x; stats5[c * 5 + 1] = b.y; stats5[c * 5 + 2] = b.z - b.x + 1; stats5[c * 5 + 3] = b.w - b.y + 1;
            stats5[c * 5 + 4] = h_area[c];
        }
    }
    if (sc.h_result[2]) return MF_ESTATE;
    if (hipMemcpy(full, d_full, P, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ignore_map, sc.ignoreMap, P, hipMemcpyDeviceToHost) != hipSuccess)
        return MF_EHIP;
    *has_new = sc.h_result[0];
    *new_class = sc.h_result[1];
    return MF_OK;
}
extern "C" int mf_k_segmentation_labels(int32_t W, int32_t H, const uint8_t* binary, const float* depth, const uint8_t* mask,
                                        const int32_t* class_ids, int32_t n_masks, const uint8_t* projected_ids, const int32_t* model_ids,
                                        const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new,
                                        const float* p, uint8_t* ignore_map, uint8_t* full, int32_t* has_new, int32_t* new_class) {
    return mf_k_label_stage(W, H, binary, depth, mask, class_ids, n_masks, projected_ids, model_ids, model_class_ids, n_models, next_model_id,
                            allow_new, p, ignore_map, full, has_new, new_class, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
}

extern "C" int mf_k_gn_solve(const double* sys29, const double* result_rt16, const float* Rprev9, const float* tprev3, double* x6_serial,
                             double* x6_wave, double* result_rt16_out, float* Rcurr9, float* tcurr3, float* stats2, void* stream) {
    if (!sys29 || !result_rt16 || !Rprev9 || !tprev3 || !x6_serial || !x6_wave || !result_rt16_out || !Rcurr9 || !tcurr3 || !stats2) return MF_EINVAL;
    const int rc = gn_solve_standalone(sys29, result_rt16, Rprev9, tprev3, x6_serial, x6_wave, result_rt16_out, Rcurr9, tcurr3, stats2, (hipStream_t)stream);
    return rc == 0 ? MF_OK : (rc == -1 ? MF_ENOMEM : MF_EHIP);
}
extern "C" int mf_k_icp_launch_form(int32_t W, int32_t H, int32_t out[5]) {
    if (!out || W <= 0 || H <= 0) return MF_EINVAL;
    const IcpForm f = icp_launch_form(W, H);
    out[0] = f.threads; out[1] = f.slots; out[2] = f.blocks; out[3] = f.chunk; out[4] = f.live;
    return MF_OK;
}
// a threshold icp_gates can bracket: not negative (its first loop would walk down to 0 and stay there), not NaN, not infinite
static bool icp_threshold_ok(float t) { return t >= 0.f && t <= 3.4028234664e38f; }
extern "C" int mf_k_icp_step_form(int32_t form, const float* Rcurr9, const float* tcurr3, const float* d_vc, const float* d_nc, const float* Rpi9,
                                  const float* tprev3, float fx, float fy, float cx, float cy, const float* d_vp, const float* d_np,
                                  float dist_thresh, float angle_thresh, int32_t W, int32_t H, float* d_out32, const int32_t* rect4_or_null,
                                  void* stream) {
    if (!Rcurr9 || !tcurr3 || !d_vc || !d_nc || !Rpi9 || !tprev3 || !d_vp || !d_np || !d_out32 || W <= 0 || H <= 0 || (W * H) % 4 || form < 0 ||
        form > 3 || (form == 2 && !rect4_or_null) || !icp_threshold_ok(dist_thresh) || !icp_threshold_ok(angle_thresh))
        return MF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float* scratch = nullptr;
    const size_t nb = (size_t)icp_geo_grid_blocks(W, H);
    const size_t bytes = nb * kIcpSlots * sizeof(float) + 2 * sizeof(GNState) + 24 * sizeof(float) + 64;
    if (hipMalloc((void**)&scratch, bytes) != hipSuccess) return MF_ENOMEM;
    char* base = reinterpret_cast<char*>(scratch);
    size_t o = nb * kIcpSlots * sizeof(float);
    o = (o + 15) & ~(size_t)15;
    GNState* st = reinterpret_cast<GNState*>(base + o);
    float* dpose = reinterpret_cast<float*>(base + o + 2 * sizeof(GNState));
    float hp[24];
    memcpy(hp, Rcurr9, 36); memcpy(hp + 9, tcurr3, 12); memcpy(hp + 12, Rpi9, 36); memcpy(hp + 21, tprev3, 12);
    (void)hipMemcpyAsync(dpose, hp, sizeof(hp), hipMemcpyHostToDevice, s);
    (void)hipStreamSynchronize(s);  // hp is a stack buffer
    int rc = 0;
    if (form == 0)
        launch_icp_step_standalone(dpose, dpose + 9, d_vc, d_nc, dpose + 12, dpose + 21, Intr{fx, fy, cx, cy}, d_vp, d_np, dist_thresh,
                                   angle_thresh, W, H, scratch, st, d_out32, s);
    else
        rc = icp_step_form_standalone(form, dpose, d_vc, d_nc, Intr{fx, fy, cx, cy}, d_vp, d_np, dist_thresh, angle_thresh, W, H, rect4_or_null,
                                      d_out32, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(scratch);
    if (rc != 0) return rc == -1 ? MF_ENOMEM : MF_EHIP;
    return launch_rc();
}
extern "C" int mf_k_icp_step(const float* Rcurr9, const float* tcurr3, const float* d_vc, const float* d_nc, const float* Rpi9,
                             const float* tprev3, float fx, float fy, float cx, float cy, const float* d_vp, const float* d_np,
                             float dist_thresh, float angle_thresh, int32_t W, int32_t H, float* d_out32, void* stream) {
    return mf_k_icp_step_form(0, Rcurr9, tcurr3, d_vc, d_nc, Rpi9, tprev3, fx, fy, cx, cy, d_vp, d_np, dist_thresh, angle_thresh, W, H, d_out32,
                              nullptr, stream);
}
// The level-0 gate image (the pose-independent tests of RGBResidual::getProducts, once per frame) from both kernels that write it: k_derivative
// on d_src, and k_rgb_pyramid on an RGB image whose three channels equal d_src -- with the intensity image that kernel derived from it, which
// the caller compares with d_src.  *pyramid_ran = 0 (and d_gate_pyramid / d_gray_pyramid untouched) at sizes the pyramid's tiling does not cover.
extern "C" int mf_k_rgb_gate(const uint8_t* d_src, int32_t W, int32_t H, const float* min_scale3, uint8_t* d_gate_single, uint8_t* d_gate_pyramid,
                             int16_t* d_dIdx, int16_t* d_dIdy, uint8_t* d_gray_pyramid, int32_t* pyramid_ran, void* stream) {
    if (!d_src || !min_scale3 || !d_gate_single || !d_gate_pyramid || !d_dIdx || !d_dIdy || !d_gray_pyramid || !pyramid_ran || W < 4 || H < 4)
        return MF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    *pyramid_ran = 0;
    launch_derivative(d_src, d_dIdx, d_dIdy, W, H, min_scale3[0], d_gate_single, s);
    if (hipStreamSynchronize(s) != hipSuccess) return MF_EHIP;
    if ((W & 3) || (H & 3)) return launch_rc();
    const size_t P = (size_t)W * H, P1 = P / 4, P2 = P / 16, PS = P + P1 + P2;
    std::vector<uint8_t> h_src(P), h_rgb(3 * P);
    if (hipMemcpy(h_src.data(), d_src, P, hipMemcpyDeviceToHost) != hipSuccess) return MF_EHIP;
    for (size_t i = 0; i < P; ++i) h_rgb[3 * i] = h_rgb[3 * i + 1] = h_rgb[3 * i + 2] = h_src[i];
    char* buf = nullptr;   // int16 dIdx[3 levels], dIdy[3 levels] | gray 1, 2 | gate 1, 2 | rgb
    if (hipMalloc((void**)&buf, 4 * PS + 2 * (P1 + P2) + 3 * P) != hipSuccess) return MF_ENOMEM;
    int16_t* dx = reinterpret_cast<int16_t*>(buf);
    int16_t* dy = dx + PS;
    uint8_t* bytes = reinterpret_cast<uint8_t*>(buf + 4 * PS);
    uint8_t* rgb = bytes + 2 * (P1 + P2);
    uint8_t* const gray[3] = {d_gray_pyramid, bytes, bytes + P1};
    uint8_t* const gate[3] = {d_gate_pyramid, bytes + P1 + P2, bytes + 2 * P1 + P2};
    int16_t* const dIdx[3] = {dx, dx + P, dx + P + P1};
    int16_t* const dIdy[3] = {dy, dy + P, dy + P + P1};
    hipError_t e = hipMemcpy(rgb, h_rgb.data(), 3 * P, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        *pyramid_ran = launch_rgb_pyramid(rgb, W, H, gray, dIdx, dIdy, gate, min_scale3, true, s) ? 1 : 0;
        e = hipStreamSynchronize(s);
    }
    (void)hipFree(buf);
    return e == hipSuccess ? launch_rc() : MF_EHIP;
}
