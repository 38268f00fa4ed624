// mf_render.inl -- headless rendering of the surfel maps: mf_render_view[_dev], mf_default_render_view, mf_sensor_render_view, mf_default_palette (kernels: mf_render.hip).
// (part of mf_context.hip, included after the model list helpers)

// Scratch of the render, allocated on the first call and freed by mf_destroy: nothing of it is shared with the frame path (the visibility list of
// the projection passes, vis_tag, stays untouched).
struct RenderScratch {
    RenderModel* d_models = nullptr; RenderModel* h_models = nullptr;   // [kMaxRenderModels], pinned staging
    float* d_palette = nullptr; float* h_palette = nullptr; int palette_cap = 0;
    hipEvent_t ev_staged = nullptr;     // the last call's staging copies have completed
    int* d_work = nullptr; size_t work_cap = 0; int* d_counts = nullptr;   // [0]: listed runs
    int* d_tile_count = nullptr; int tiles_cap = 0;
    uint2* d_entries = nullptr; size_t entries_cap = 0;
    int* h_overflow = nullptr;          // pinned: a tile list ran over its slice since the last call
    uint8_t* d_rgba = nullptr; float* d_depth = nullptr; int* d_model = nullptr; size_t pixels_cap = 0;   // mf_render_view's device outputs
    ~RenderScratch() {
        for (void* p : {(void*)d_models, (void*)d_palette, (void*)d_work, (void*)d_counts, (void*)d_tile_count, (void*)d_entries, (void*)d_rgba,
                        (void*)d_depth, (void*)d_model})
            if (p) (void)hipFree(p);
        for (void* p : {(void*)h_models, (void*)h_palette, (void*)h_overflow})
            if (p) (void)hipHostFree(p);
        if (ev_staged) (void)hipEventDestroy(ev_staged);
    }
};
static void render_free(RenderScratch* r) { delete r; }

constexpr int kRenderMaxSide = 4096;
constexpr int kDefaultPaletteSize = 64;
constexpr size_t kRenderEntriesInitial = (size_t)1 << 24, kRenderEntriesMax = (size_t)1 << 27;

static int render_fail(mf_ctx* c, const char* why) { c->err = why; return MF_EINVAL; }

// the library's own palette: hues on the golden-angle walk, three saturations, two values (not upstream's color_table.glsl)
static void default_palette_entry(int k, float* rgb) {
    const double h = fmod(0.08 + 0.6180339887498949 * k, 1.0) * 6.0;
    const double s = k % 3 == 0 ? 0.85 : (k % 3 == 1 ? 0.65 : 0.5), v = (k / 3) % 2 == 0 ? 0.95 : 0.75;
    const int sector = (int)h % 6;
    const double f = h - floor(h), p = v * (1 - s), q = v * (1 - s * f), t = v * (1 - s * (1 - f));
    double r, g, b;
    switch (sector) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
    rgb[0] = (float)r; rgb[1] = (float)g; rgb[2] = (float)b;
}
extern "C" int mf_default_palette(float* out, int32_t capacity, int32_t* n) {
    if (!n || capacity < 0) return MF_EINVAL;
    const int m = out ? std::min(capacity, kDefaultPaletteSize) : kDefaultPaletteSize;
    if (out)
        for (int k = 0; k < m; ++k) default_palette_entry(k, out + 3 * k);
    *n = m;
    return MF_OK;
}

extern "C" int mf_default_render_view(mf_ctx* c, int32_t width, int32_t height, int32_t icl, mf_render_view_t* out) {
    settle(c);
    if (!c || !out) return MF_EINVAL;
    if (width < 1 || height < 1 || width > kRenderMaxSide || height > kRenderMaxSide) return render_fail(c, "render size outside 1 .. 4096");
    float pose[16];
    int rc = mf_get_pose(c, 0, pose);
    if (rc != MF_OK) return rc;
    memset(out, 0, sizeof(*out));
    out->width = width; out->height = height;
    out->fx = out->fy = 420.f; out->cx = width / 2.0f; out->cy = height / 2.0f;   // GUI.h:73
    out->near_z = 0.1f; out->far_z = 1000.f;
    // MainController.cpp:610-640: eye = t - 0.2 forward, the view's axes those of the camera (x right, y down, z forward); with the ICL up
    // vector x and y change sign
    const double sgn = icl ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) {
        out->pose16[0 * 4 + r] = (float)(sgn * pose[0 * 4 + r]);
        out->pose16[1 * 4 + r] = (float)(sgn * pose[1 * 4 + r]);
        out->pose16[2 * 4 + r] = pose[2 * 4 + r];
        out->pose16[12 + r] = (float)((double)pose[12 + r] - 0.2 * (double)pose[2 * 4 + r]);
    }
    out->pose16[15] = 1.f;
    out->background_color_type = out->object_color_type = 2;
    out->draw_background = out->draw_objects = 1;
    out->clear_rgba[0] = out->clear_rgba[1] = out->clear_rgba[2] = out->clear_rgba[3] = 255;
    return MF_OK;
}

extern "C" int mf_sensor_render_view(mf_ctx* c, mf_render_view_t* out) {
    settle(c);
    if (!c || !out) return MF_EINVAL;
    float pose[16];
    int rc = mf_get_pose(c, 0, pose);
    if (rc != MF_OK) return rc;
    memset(out, 0, sizeof(*out));
    out->width = c->W; out->height = c->H;
    out->fx = c->K.fx; out->fy = c->K.fy; out->cx = c->K.cx; out->cy = c->K.cy;
    out->near_z = 0.01f; out->far_z = 1000.f;
    memcpy(out->pose16, pose, sizeof(pose));
    out->background_color_type = out->object_color_type = 2;
    out->draw_background = out->draw_objects = 1;
    out->clear_rgba[3] = 255;
    return MF_OK;
}

static int render_enqueue(mf_ctx* c, const mf_render_view_t* v, const float* palette, int32_t n_palette, uint8_t* d_rgba, float* d_depth,
                          int32_t* d_model) {
    if (!c) return MF_EINVAL;
    if (!v || !d_rgba) return render_fail(c, "mf_render_view: null view or colour output");
    if (v->width < 1 || v->height < 1 || v->width > kRenderMaxSide || v->height > kRenderMaxSide) return render_fail(c, "render size outside 1 .. 4096");
    if (!(std::isfinite(v->fx) && std::isfinite(v->fy) && std::isfinite(v->cx) && std::isfinite(v->cy) && v->fx != 0.f && v->fy != 0.f))
        return render_fail(c, "render intrinsics must be finite, fx and fy non-zero");
    if (!(v->near_z > 0.f && v->far_z > v->near_z && std::isfinite(v->far_z))) return render_fail(c, "render depth range: 0 < near < far required");
    for (int q = 0; q < 16; ++q)
        if (!std::isfinite(v->pose16[q])) return render_fail(c, "render pose is not finite");
    for (int q = 0; q < 8; ++q)
        if (v->reserved[q] != 0) return render_fail(c, "render view: reserved fields must be zero");
    if (n_palette < 0 || (!palette && n_palette != 0)) return render_fail(c, "render palette: n < 0, or entries without a pointer");
    const int nm_all = (int)c->models.size();
    if (nm_all == 0) return render_fail(c, "no model to render");
    if (v->model_mask) {
        for (int b = nm_all; b < 64; ++b)
            if ((v->model_mask >> b) & 1ull) return render_fail(c, "render model mask names a model that does not exist");
    }
    const bool labels = !v->draw_points && (v->background_color_type == 4 || v->object_color_type == 4);
    if (labels && palette && n_palette == 0) return render_fail(c, "colour type 4 needs a palette with at least one entry");
    if (!c->render) c->render = new RenderScratch();
    RenderScratch& r = *c->render;
    hipStream_t s = c->stream;
    if (!r.d_models) {
        MF_HIP(c, hipMalloc(&r.d_models, kMaxRenderModels * sizeof(RenderModel)));
        MF_HIP(c, hipHostMalloc(&r.h_models, kMaxRenderModels * sizeof(RenderModel)));
        MF_HIP(c, hipHostMalloc(&r.h_overflow, sizeof(int)));
        *r.h_overflow = 0;
        MF_HIP(c, hipMalloc(&r.d_counts, 4 * sizeof(int)));
        MF_HIP(c, hipEventCreateWithFlags(&r.ev_staged, hipEventDisableTiming));
        MF_HIP(c, hipEventRecord(r.ev_staged, s));
    }
    MF_HIP(c, hipEventSynchronize(r.ev_staged));   // the pinned staging of the previous call has been copied
    // the drawn models in draw order: the background, then the objects in list order
    int nm = 0;
    size_t base = 0, work = 0;
    int max_runs = 0;
    for (int i = 0; i < nm_all; ++i) {
        const bool wanted = (i == 0 ? v->draw_background : v->draw_objects) && (v->model_mask == 0 || (i < 64 && ((v->model_mask >> i) & 1ull)));
        if (!wanted) continue;
        if (nm == kMaxRenderModels) return render_fail(c, "more than 256 models in one render");
        ModelState& m = *c->models[i];
        RenderModel& d = r.h_models[nm];
        memset(&d, 0, sizeof(d));
        d.s = m.surf[m.cur]; d.frame = m.d_frame; d.pose = m.d_pose;
        d.base = (unsigned)base;
        const int chunks = (m.cap + kRun - 1) / kRun;
        d.max_runs = std::max(chunks, (int)run_table_runs(m.cap, c->P));
        d.thr = m.confThr; d.class_id = m.classID; d.index = i; d.is_background = i == 0 ? 1 : 0;
        d.color_type = i == 0 ? v->background_color_type : v->object_color_type;
        base += (size_t)m.cap;
        work += (size_t)d.max_runs;
        max_runs = std::max(max_runs, d.max_runs);
        ++nm;
    }
    if (base >= 0xFFFFFFFFull) return render_fail(c, "the drawn models hold more than 2^32 - 1 surfel slots");
    // palette
    int npal = n_palette;
    const float* pal = palette;
    float defpal[3 * kDefaultPaletteSize];
    if (!palette) { npal = kDefaultPaletteSize; for (int k = 0; k < npal; ++k) default_palette_entry(k, defpal + 3 * k); pal = defpal; }
    if (npal > r.palette_cap) {
        MF_HIP(c, hipStreamSynchronize(s));
        if (r.d_palette) MF_HIP(c, hipFree(r.d_palette));
        if (r.h_palette) MF_HIP(c, hipHostFree(r.h_palette));
        r.d_palette = nullptr; r.h_palette = nullptr; r.palette_cap = 0;
        MF_HIP(c, hipMalloc(&r.d_palette, (size_t)3 * npal * sizeof(float)));
        MF_HIP(c, hipHostMalloc(&r.h_palette, (size_t)3 * npal * sizeof(float)));
        r.palette_cap = npal;
    }
    if (npal > 0) memcpy(r.h_palette, pal, (size_t)3 * npal * sizeof(float));
    // list / tile buffers
    const int tilesX = (v->width + 15) / 16, tilesY = (v->height + 15) / 16, nt = tilesX * tilesY;
    if (*r.h_overflow && r.entries_cap < kRenderEntriesMax) {   // a tile of an earlier call scanned every listed run: larger slices from now on
        MF_HIP(c, hipStreamSynchronize(s));
        MF_HIP(c, hipFree(r.d_entries));
        r.d_entries = nullptr;
        r.entries_cap = std::min(kRenderEntriesMax, r.entries_cap * 2);
    }
    *r.h_overflow = 0;
    if (!r.d_entries) {
        if (!r.entries_cap) r.entries_cap = kRenderEntriesInitial;
        MF_HIP(c, hipMalloc(&r.d_entries, r.entries_cap * sizeof(uint2)));
    }
    if (work > r.work_cap) {
        MF_HIP(c, hipStreamSynchronize(s));
        if (r.d_work) MF_HIP(c, hipFree(r.d_work));
        r.d_work = nullptr;
        MF_HIP(c, hipMalloc(&r.d_work, work * sizeof(int)));
        r.work_cap = work;
    }
    if (nt > r.tiles_cap) {
        MF_HIP(c, hipStreamSynchronize(s));
        if (r.d_tile_count) MF_HIP(c, hipFree(r.d_tile_count));
        r.d_tile_count = nullptr;
        MF_HIP(c, hipMalloc(&r.d_tile_count, (size_t)nt * sizeof(int)));
        r.tiles_cap = nt;
    }
    if (nm > 0) MF_HIP(c, hipMemcpyAsync(r.d_models, r.h_models, (size_t)nm * sizeof(RenderModel), hipMemcpyHostToDevice, s));
    if (npal > 0) MF_HIP(c, hipMemcpyAsync(r.d_palette, r.h_palette, (size_t)3 * npal * sizeof(float), hipMemcpyHostToDevice, s));
    MF_HIP(c, hipEventRecord(r.ev_staged, s));
    MF_HIP(c, hipMemsetAsync(r.d_counts, 0, 4 * sizeof(int), s));
    MF_HIP(c, hipMemsetAsync(r.d_tile_count, 0, (size_t)nt * sizeof(int), s));
    // world -> view from camera -> world (column-major), in double
    RenderView rv;
    {
        double R[9], t[3];
        for (int row = 0; row < 3; ++row) {
            for (int col = 0; col < 3; ++col) R[row * 3 + col] = v->pose16[col * 4 + row];
            t[row] = v->pose16[12 + row];
        }
        for (int row = 0; row < 3; ++row) {
            double tt = 0.0;
            for (int col = 0; col < 3; ++col) { rv.Vi[row * 4 + col] = (float)R[col * 3 + row]; tt -= R[col * 3 + row] * t[col]; }
            rv.Vi[row * 4 + 3] = (float)tt;
        }
    }
    RenderArgs a;
    memset(&a, 0, sizeof(a));
    a.models = r.d_models; a.n_models = nm;
    a.W = v->width; a.H = v->height; a.k = Intr{v->fx, v->fy, v->cx, v->cy}; a.near_z = v->near_z; a.far_z = v->far_z;
    a.drawUnstable = v->draw_unstable != 0; a.drawPoints = v->draw_points != 0; a.drawWindow = v->draw_window != 0; a.timeDelta = c->cfg.time_delta;
    a.tick_frame = c->models[0]->d_frame;
    a.palette = r.d_palette; a.n_palette = std::max(npal, 1);
    a.clear = make_uchar4(v->clear_rgba[0], v->clear_rgba[1], v->clear_rgba[2], v->clear_rgba[3]);
    a.work = r.d_work; a.work_count = r.d_counts;
    a.tilesX = tilesX; a.tilesY = tilesY; a.tile_cap = (int)std::min<size_t>(r.entries_cap / (size_t)nt, 1u << 30);
    a.tile_count = r.d_tile_count; a.entries = r.d_entries; a.overflow = r.h_overflow;
    a.out_rgba = reinterpret_cast<uchar4*>(d_rgba); a.out_depth = d_depth; a.out_model = d_model;
    if (nm == 0) max_runs = 1;
    launch_render(a, rv, c->models[0]->d_pose, std::max(max_runs, 1), s);
    return check_launch(c);
}

extern "C" int mf_render_view_dev(mf_ctx* c, const mf_render_view_t* v, const float* palette, int32_t n_palette, uint8_t* d_rgba, float* d_depth,
                                  int32_t* d_model) {
    settle(c);
    return render_enqueue(c, v, palette, n_palette, d_rgba, d_depth, d_model);
}

extern "C" int mf_render_view(mf_ctx* c, const mf_render_view_t* v, const float* palette, int32_t n_palette, uint8_t* out_rgba, float* out_depth,
                              int32_t* out_model) {
    settle(c);
    if (!c) return MF_EINVAL;
    if (!v || !out_rgba) return render_fail(c, "mf_render_view: null view or colour output");
    if (v->width < 1 || v->height < 1 || v->width > kRenderMaxSide || v->height > kRenderMaxSide) return render_fail(c, "render size outside 1 .. 4096");
    if (!c->render) c->render = new RenderScratch();
    RenderScratch& r = *c->render;
    const size_t P = (size_t)v->width * v->height;
    if (P > r.pixels_cap) {
        MF_HIP(c, hipStreamSynchronize(c->stream));
        for (void** p : {(void**)&r.d_rgba, (void**)&r.d_depth, (void**)&r.d_model})
            if (*p) { MF_HIP(c, hipFree(*p)); *p = nullptr; }
        r.pixels_cap = 0;
        MF_HIP(c, hipMalloc(&r.d_rgba, P * 4));
        MF_HIP(c, hipMalloc(&r.d_depth, P * sizeof(float)));
        MF_HIP(c, hipMalloc(&r.d_model, P * sizeof(int)));
        r.pixels_cap = P;
    }
    int rc = render_enqueue(c, v, palette, n_palette, r.d_rgba, out_depth ? r.d_depth : nullptr, out_model ? r.d_model : nullptr);
    if (rc != MF_OK) return rc;
    MF_HIP(c, hipMemcpyAsync(out_rgba, r.d_rgba, P * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_depth) MF_HIP(c, hipMemcpyAsync(out_depth, r.d_depth, P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_model) MF_HIP(c, hipMemcpyAsync(out_model, r.d_model, P * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return mf_sync(c);
}
