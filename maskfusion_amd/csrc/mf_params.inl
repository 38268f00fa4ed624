// mf_params.inl -- part of mf_context.hip: the ONE table of the keys of mf_set_param / mf_get_param, and the two functions.
//
// A key is a row: where its value lives, its type, its legal values, who may read and write it, and what else setting it does.  The rows stand in
// the order of the list above mf_set_param in include/maskfusion_amd.h, which says what each position means (the members' comments in
// struct Switches, mf_context.hip, say what it does to the implementation).  A legal set is written here and in that header, nowhere else.

enum ParamHome : uint8_t { kInCfg, kInSeg, kInSw, kComputed };   // mf_ctx::cfg | ::seg | ::sw (SplatTuning included) | no storage: the row's get / set do the work
enum ParamType : uint8_t { kFlag, kInt, kFloat };                // bool, stored as value != 0 | int32 | float
enum ParamAccess : uint8_t { kReadWrite, kReadOnly, kWriteOnly };
struct ParamRow {
    const char* key;
    ParamHome home; size_t off;                  // kComputed: `off` is the row's own business (an index for a getter that serves several keys)
    ParamType type;
    ParamAccess access;
    int legal[6];                                // the values mf_set_param accepts, ending with a 0; {}: any
    int (*after_set)(mf_ctx*);                   // runs behind the store; its return value is the call's
    int (*get)(mf_ctx*, const ParamRow&, double*);   // in place of the load
    int (*set)(mf_ctx*, const ParamRow&, double);    // in place of the check, the store and after_set
};

// ---- side effects of setting a key ----
static int drop_visibility_list(mf_ctx* c) { c->vis_tag.model = nullptr; return MF_OK; }   // the cached list was culled under the other position
static int clear_pass_timings(mf_ctx* c) {
    for (int q = 0; q < MF_N_PASSES; ++q) { c->pass_recorded[q] = false; c->pass_ms[q] = 0.f; }
    return MF_OK;
}
static int push_weight_literal(mf_ctx* c) {   // PoseDev::weightLiteral of every live and pooled model
    for (auto& m : c->models) hipLaunchKernelGGL(k_set_weight_literal, dim3(1), dim3(64), 0, c->stream, m->d_pose, c->sw.weight_literal ? 1 : 0, m->h_pose);
    for (auto& m : c->pool) hipLaunchKernelGGL(k_set_weight_literal, dim3(1), dim3(64), 0, c->stream, m->d_pose, c->sw.weight_literal ? 1 : 0, m->h_pose);
    return check_launch(c);
}
static int set_host_async(mf_ctx* c, const ParamRow&, double value) {   // both streams are idle before the form of mf_process_frame changes
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipStreamSynchronize(c->stream_in) != hipSuccess) return MF_EHIP;
    c->sw.host_async = value != 0;
    return MF_OK;
}
static int set_splat_profile(mf_ctx* c, const ParamRow&, double value) {   // the stamps' buffer is allocated on first use
    if (value != 0 && !c->d_splat_prof) {
        if (hipMalloc(&c->d_splat_prof, splat_tiles_scratch_ints(c->W, c->H) * 8 * sizeof(unsigned long long)) != hipSuccess) return MF_ENOMEM;
    }
    c->sw.splat_prof_on = value != 0;
    return MF_OK;
}
static int set_confidence(mf_ctx* c, const ParamRow&, double value) { c->cfg.conf_global = (float)value; c->models[0]->confThr = (float)value; return MF_OK; }
static int get_confidence(mf_ctx* c, const ParamRow&, double* value) { *value = c->models[0]->confThr; return MF_OK; }
static int set_tile_entries(mf_ctx* c, const ParamRow& p, double value) {   // shrinks the tile lists (never beyond what was allocated) to force the overflow path
    const long long v = (long long)value;
    if (v < 1 || v > c->tile_entries_alloc) { c->err = std::string(p.key) + ": the legal values are 1 to " + std::to_string(c->tile_entries_alloc); return MF_EINVAL; }
    c->tile_entries_cap = (int)v;
    return MF_OK;
}
static int get_tile_entries(mf_ctx* c, const ParamRow&, double* value) { *value = c->tile_entries_cap; return MF_OK; }
// ---- actions ----
static int reset_host_profile(mf_ctx* c, const ParamRow&, double) { for (double& v : c->host_us) v = 0; c->host_calls = 0; return MF_OK; }
static int rebuild_run_table(mf_ctx* c, const ParamRow&, double) {   // tooling: the background's run table from scratch (what an upload / Model::initialise does)
    // fixed runs over slots [0, count) describe a DENSE buffer only: a sparse one is compacted first, and the host's bounds start afresh
    ModelState& bg = *c->models[0];
    require_dense(c, bg);
    MF_HIP(c, hipStreamSynchronize(c->stream));   // (the exact count: the pinned mirror as of the last clean pass / the compaction)
    launch_run_table(bg.surf[bg.cur], bg.d_frame, c->stream);
    bg.fresh_table(bg.cur, (long)*bg.h_count);
    c->vis_tag.model = nullptr;
    return check_launch(c);
}
// ---- read-only taps ----
static int get_index_texel_bytes(mf_ctx* c, const ParamRow&, double* value) { *value = c->iclean_is_tap16 ? 16 : 32; return MF_OK; }   // the form "index_packed" holds
static int get_deferred_frames(mf_ctx* c, const ParamRow&, double* value) { *value = (double)c->deferred_frames; return MF_OK; }
static int get_fused_head_frames(mf_ctx* c, const ParamRow&, double* value) { *value = (double)c->fused_head_frames; return MF_OK; }
static int get_pyramid_fixups(mf_ctx* c, const ParamRow&, double* value) {   // fused heads whose fill-in decision was 1: the fix-up launch rebuilt the model-side pyramid there
    int v = 0;
    MF_HIP(c, hipStreamSynchronize(c->stream));
    MF_HIP(c, hipMemcpy(&v, c->d_pyramid_fixups, sizeof(int), hipMemcpyDeviceToHost));
    *value = v;
    return MF_OK;
}
static int get_densify_count(mf_ctx* c, const ParamRow&, double* value) { *value = (float)c->densify_count; return MF_OK; }
enum { kRunsVisible, kRunsClean, kRunsBackground };   // ParamRow::off of the rows that get_run_count serves
static int get_run_count(mf_ctx* c, const ParamRow& p, double* value) {   // test taps: size of the last visibility list / of the last clean list / of the background's run table
    MF_HIP(c, hipStreamSynchronize(c->stream));
    int v = 0;
    if (p.off == kRunsVisible) MF_HIP(c, hipMemcpy(&v, c->d_vis_count, sizeof(int), hipMemcpyDeviceToHost));
    else if (p.off == kRunsClean) MF_HIP(c, hipMemcpy(&v, c->d_clean_count, sizeof(int), hipMemcpyDeviceToHost));
    else { FrameDev f; MF_HIP(c, hipMemcpy(&f, c->models[0]->d_frame, sizeof(FrameDev), hipMemcpyDeviceToHost)); v = f.runs; }
    *value = v;
    return MF_OK;
}
static int get_unstamped_runs(mf_ctx* c, const ParamRow&, double* value) {   // test tap: live runs of the background's table that carry "holds a time stamp <= 0" (k_cull_clean lists them)
    MF_HIP(c, hipStreamSynchronize(c->stream));
    ModelState& bg = *c->models[0];
    FrameDev f; MF_HIP(c, hipMemcpy(&f, bg.d_frame, sizeof(FrameDev), hipMemcpyDeviceToHost));
    const size_t cap_runs = run_table_runs((long)bg.cap, (long)c->P);
    const size_t runs = bg.table_valid ? std::min((size_t)std::max(f.runs, 0), cap_runs) : 0;
    std::vector<int4> box(kBoxStride * runs);
    if (runs) MF_HIP(c, hipMemcpy(box.data(), bg.surf[bg.cur].box, box.size() * sizeof(int4), hipMemcpyDeviceToHost));
    int v = 0;
    for (size_t r = 0; r < runs; ++r) v += (box[kBoxStride * r + 2].x > 0 && box[kBoxStride * r + 2].z != 0) ? 1 : 0;
    *value = v;
    return MF_OK;
}
// mean host microseconds per mf_process_frame call since the last "hostProfileReset": mf_ctx::host_us[ParamRow::off]
static int get_host_us(mf_ctx* c, const ParamRow& p, double* value) { *value = c->host_calls ? c->host_us[p.off] / c->host_calls : 0; return MF_OK; }

static const ParamRow kParamTable[] = {
    // ---- reference parameters: the per-frame setters of MaskFusion ----
    {"depthCutoff", kInCfg, offsetof(mf_config, depth_cutoff), kFloat},
    {"icpWeight", kInCfg, offsetof(mf_config, icp_weight), kFloat},
    {"confidenceThreshold", kComputed, 0, kFloat, kReadWrite, {}, nullptr, get_confidence, set_confidence},   // cfg.conf_global and the background's confThr
    {"outlierCoefficient", kInCfg, offsetof(mf_config, outlier_coefficient), kFloat},
    {"maxDepthProcessed", kInCfg, offsetof(mf_config, max_depth_processed), kFloat},
    {"fastOdom", kInCfg, offsetof(mf_config, fast_odom), kInt},
    {"so3", kInCfg, offsetof(mf_config, so3), kInt},
    {"rgbOnly", kInCfg, offsetof(mf_config, rgb_only), kInt},
    {"pyramid", kInCfg, offsetof(mf_config, pyramid), kInt},
    {"timeDelta", kInCfg, offsetof(mf_config, time_delta), kInt},
    {"enableMultipleModels", kInCfg, offsetof(mf_config, enable_multiple_models), kInt},
    {"trackAllModels", kInCfg, offsetof(mf_config, track_all_models), kInt},
    {"modelSpawnOffset", kInCfg, offsetof(mf_config, model_spawn_offset), kInt},
    {"keepInactiveModels", kInSw, offsetof(Switches, keep_inactive), kFlag},
    {"enableSmartModelDelete", kInSw, offsetof(Switches, smart_delete), kFlag},
    {"modelKeepMinSurfels", kInSw, offsetof(Switches, keep_min_surfels), kInt},
    {"modelKeepConfThreshold", kInSw, offsetof(Switches, keep_conf), kFloat},
    // ---- segmentation parameters ----
    {"newModelMinRelativeSize", kInSeg, offsetof(SegParams, minRelSizeNew), kFloat},
    {"newModelMaxRelativeSize", kInSeg, offsetof(SegParams, maxRelSizeNew), kFloat},
    {"mfThreshold", kInSeg, offsetof(SegParams, threshold), kFloat},
    {"mfWeightDistance", kInSeg, offsetof(SegParams, weightDistance), kFloat},
    {"mfWeightConvexity", kInSeg, offsetof(SegParams, weightConvexity), kFloat},
    {"mfMorphEdgeIterations", kInSeg, offsetof(SegParams, morphEdgeIterations), kInt},
    {"mfMorphEdgeRadius", kInSeg, offsetof(SegParams, morphEdgeRadius), kInt},
    {"mfMorphMaskIterations", kInSeg, offsetof(SegParams, morphMaskIterations), kInt},
    {"mfMorphMaskRadius", kInSeg, offsetof(SegParams, morphMaskRadius), kInt},
    // ---- implementation switches ----
    {"splatTiles", kInSw, offsetof(Switches, splat_tiles), kFlag},
    {"globalTiles", kInSw, offsetof(Switches, global_tiles), kFlag},
    {"gpuLabels", kInSw, offsetof(Switches, gpu_labels), kFlag},
    {"batchTracking", kInSw, offsetof(Switches, batch_tracking), kFlag},
    {"batchSolveInPixelPass", kInSw, offsetof(Switches, batch_solve_fused), kFlag},
    {"slabCulling", kInSw, offsetof(Switches, slab_culling), kFlag},
    {"earlyBackgroundFusion", kInSw, offsetof(Switches, early_bg_fusion), kFlag},
    {"cleanTap16", kInSw, offsetof(Switches, clean_tap16), kFlag},
    {"cleanTapGroup", kInSw, offsetof(Switches, clean_tap_group), kInt, kReadWrite, {1, 3, 9}},
    {"maskFreeClean", kInSw, offsetof(Switches, mask_free_clean), kFlag},
    {"fuseLanes", kInSw, offsetof(Switches, fuse_lanes), kInt, kReadWrite, {1, 4}},
    {"cleanLiteralWindow", kInSw, offsetof(Switches, clean_literal), kFlag},
    {"objectSmallGrids", kInSw, offsetof(Switches, object_small_grids), kFlag},
    {"objectScatterSplat", kInSw, offsetof(Switches, object_scatter_splat), kFlag},
    {"batchObjectPasses", kInSw, offsetof(Switches, batch_objects), kFlag},
    {"objectStream", kInSw, offsetof(Switches, object_stream), kFlag},
    {"cullRuns", kInSw, offsetof(Switches, cull_runs), kFlag, kReadWrite, {}, drop_visibility_list},
    {"literalFusionWeight", kInSw, offsetof(Switches, weight_literal), kFlag, kReadWrite, {}, push_weight_literal},
    {"frameToFrameRGB", kInSw, offsetof(Switches, ftf_rgb), kFlag},
    {"objectBoundingBoxLimit", kInSw, offsetof(Switches, bbox_limit), kFlag},
    {"fusedRgbPyramid", kInSw, offsetof(Switches, fused_rgb_pyramid), kFlag},
    {"fusedPreprocessLaunch", kInSw, offsetof(Switches, fused_preprocess), kFlag},
    {"deferPredict", kInSw, offsetof(Switches, defer_predict), kFlag},
    {"fusedBinFilter", kInSw, offsetof(Switches, fused_bin_filter), kFlag},
    {"fusedFramePyramids", kInSw, offsetof(Switches, fused_frame_pyramids), kFlag},
    {"tilePyramid", kInSw, offsetof(Switches, tile_pyramid), kFlag},
    {"fusedTilePyramid", kInSw, offsetof(Switches, fused_tile_pyramid), kFlag},
    {"hostInputAsync", kInSw, offsetof(Switches, host_async), kFlag, kReadWrite, {}, nullptr, nullptr, set_host_async},
    {"hostLockstep", kInSw, offsetof(Switches, host_lockstep), kFlag},
    {"hostWaitUpload", kInSw, offsetof(Switches, host_wait_upload), kFlag},
    {"modelApiPackedIndex", kInSw, offsetof(Switches, model_api_packed), kFlag},
    // ---- tuning knobs ----
    {"bigMapElements", kInSw, offsetof(Switches, big_map_elements), kInt, kReadWrite, {}, drop_visibility_list},
    {"inPlaceElements", kInSw, offsetof(Switches, in_place_elements), kInt},
    {"tileHeight", kInSw, offsetof(Switches, splat_tune.tile_h), kInt, kReadWrite, {16, 20, 24, 32}},            // tiles of 16 pixels by that many rows
    {"tileThreads", kInSw, offsetof(Switches, splat_tune.tile_threads), kInt, kReadWrite, {256, 320, 384, 512, 1024}},   // threads per tile workgroup
    {"spriteLanes", kInSw, offsetof(Switches, splat_tune.sprite_lanes), kInt, kReadWrite, {1, 2, 4, 8, 16}},     // lanes per sprite in the tile z-test
    // ---- test knobs and actions ----
    {"densifyEvery", kInSw, offsetof(Switches, densify_every), kInt},
    {"splatTileEntries", kComputed, 0, kInt, kReadWrite, {}, nullptr, get_tile_entries, set_tile_entries},
    {"timings", kInSw, offsetof(Switches, timings_on), kFlag},
    {"passTimings", kInSw, offsetof(Switches, pass_timings_on), kFlag, kReadWrite, {}, clear_pass_timings},
    {"icpProfile", kInSw, offsetof(Switches, icp_prof_on), kFlag},
    {"splatProfile", kInSw, offsetof(Switches, splat_prof_on), kFlag, kReadWrite, {}, nullptr, nullptr, set_splat_profile},
    {"hostProfileReset", kComputed, 0, kFlag, kWriteOnly, {}, nullptr, nullptr, reset_host_profile},
    {"rebuildRunTable", kComputed, 0, kFlag, kWriteOnly, {}, nullptr, nullptr, rebuild_run_table},
    // ---- read-only taps ----
    {"indexPackedTexelBytes", kComputed, 0, kInt, kReadOnly, {}, nullptr, get_index_texel_bytes},
    {"deferredFrames", kComputed, 0, kInt, kReadOnly, {}, nullptr, get_deferred_frames},
    {"fusedHeadFrames", kComputed, 0, kInt, kReadOnly, {}, nullptr, get_fused_head_frames},
    {"pyramidFixupFrames", kComputed, 0, kInt, kReadOnly, {}, nullptr, get_pyramid_fixups},
    {"densifyCount", kComputed, 0, kInt, kReadOnly, {}, nullptr, get_densify_count},
    {"cleanRuns", kComputed, kRunsClean, kInt, kReadOnly, {}, nullptr, get_run_count},
    {"visibleRuns", kComputed, kRunsVisible, kInt, kReadOnly, {}, nullptr, get_run_count},
    {"backgroundRuns", kComputed, kRunsBackground, kInt, kReadOnly, {}, nullptr, get_run_count},
    {"unstampedRuns", kComputed, 0, kInt, kReadOnly, {}, nullptr, get_unstamped_runs},
    {"hostStageUs", kComputed, 0, kFloat, kReadOnly, {}, nullptr, get_host_us},     // wait for the slot + staging copy
    {"hostUploadUs", kComputed, 1, kFloat, kReadOnly, {}, nullptr, get_host_us},    // upload enqueue
    {"hostEnqueueUs", kComputed, 2, kFloat, kReadOnly, {}, nullptr, get_host_us},   // frame enqueue
    {"hostCallUs", kComputed, 3, kFloat, kReadOnly, {}, nullptr, get_host_us},      // the whole call
    {"hostWaitUs", kComputed, 4, kFloat, kReadOnly, {}, nullptr, get_host_us},      // the wait alone
};

// the key's row and where its value lives; an MF_EINVAL of either function leaves "<key>: <why>" in mf_last_error
static int refuse_param(mf_ctx* c, const char* key, const std::string& why) { c->err = std::string(key) + ": " + why; return MF_EINVAL; }
static const ParamRow* find_param(const char* key) {
    for (const ParamRow& p : kParamTable)
        if (!strcmp(key, p.key)) return &p;
    return nullptr;
}
static char* param_home(mf_ctx* c, const ParamRow& p) {
    return (p.home == kInCfg ? reinterpret_cast<char*>(&c->cfg) : p.home == kInSeg ? reinterpret_cast<char*>(&c->seg) : reinterpret_cast<char*>(&c->sw)) + p.off;
}

extern "C" int mf_set_param(mf_ctx* c, const char* key, double value) {
    settle(c);
    if (!c || !key) return MF_EINVAL;
    const ParamRow* p = find_param(key);
    if (!p) return refuse_param(c, key, "unknown parameter");
    if (p->access == kReadOnly) return refuse_param(c, key, "read-only");
    if (p->set) return p->set(c, *p, value);
    if (p->legal[0]) {
        std::string list;
        bool ok = false;
        for (int q = 0; q < 6 && p->legal[q]; ++q) { ok = ok || (int)value == p->legal[q]; list += (q ? ", " : "") + std::to_string(p->legal[q]); }
        if (!ok) return refuse_param(c, key, "the legal values are " + list);
    }
    char* at = param_home(c, *p);
    if (p->type == kFlag) *reinterpret_cast<bool*>(at) = value != 0;
    else if (p->type == kInt) *reinterpret_cast<int32_t*>(at) = (int32_t)value;
    else *reinterpret_cast<float*>(at) = (float)value;
    return p->after_set ? p->after_set(c) : MF_OK;
}
extern "C" int mf_get_param(mf_ctx* c, const char* key, double* value) {
    settle(c);
    if (!c || !key || !value) return MF_EINVAL;
    const ParamRow* p = find_param(key);
    if (!p) return refuse_param(c, key, "unknown parameter");
    if (p->access == kWriteOnly) return refuse_param(c, key, "write-only");
    if (p->get) return p->get(c, *p, value);
    const char* at = param_home(c, *p);
    if (p->type == kFlag) *value = *reinterpret_cast<const bool*>(at) ? 1 : 0;
    else if (p->type == kInt) *value = (double)*reinterpret_cast<const int32_t*>(at);
    else *value = (double)*reinterpret_cast<const float*>(at);
    return MF_OK;
}
