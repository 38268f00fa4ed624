// mf_session.inl -- mf_session_save / mf_session_load / mf_session_info / mf_state_digest: a context's state as a file (kernels: mf_session.hip;
// the format: include/maskfusion_amd.h "Sessions"; which member is saved, re-derived or scratch: DESIGN.md "Sessions").
// (part of mf_context.hip, included last: it walks mf_ctx and ModelState member by member)

namespace {

constexpr char kSessionMagic[8] = {'M', 'F', 'S', 'E', 'S', 'S', 'N', '1'};
constexpr int kSessionChunk = 1 << 18;     // surfels per staged chunk: 12 MB of records
struct SessionHeader {
    char magic[8];
    uint32_t version, pose_bytes, frame_bytes, run;
    int32_t width, height, n_models, tick;
    uint64_t user_bytes;
    uint32_t n_sections, config_bytes;
    int64_t frames;
};
struct SessionEntry {
    char name[32];
    int32_t owner; uint32_t zero;
    uint64_t offset, bytes, digest;
};
static_assert(sizeof(SessionHeader) == 64 && sizeof(SessionEntry) == 64, "the documented layout (maskfusion_amd.h)");

// the device-resident sections, in the order of mf_state_digest's words (maskfusion_amd.h: MF_STATE_CONTEXT_SECTIONS, MF_STATE_MODEL_SECTIONS)
const char* const kCtxSections[MF_STATE_CONTEXT_SECTIONS] = {"segmentation", "ignore_map", "depthF0", "depthF1", "depthF2", "gray00", "gray01", "gray02",
                                                            "gray10", "gray11", "gray12", "frame_rgb", "frame_depth", "frame_mask"};
const char* const kModelSections[MF_STATE_MODEL_SECTIONS] = {"surfels", "pose", "frame", "pred_vertex", "pred_normal", "pred_image", "pred_time", "pred_gray",
                                                            "fill_gray", "pose_log", "vmap_g0", "nmap_g0", "vmap_g1", "nmap_g1", "vmap_g2", "nmap_g2"};

// a host section's bytes, written and read field by field
struct SessWriter {
    std::vector<uint8_t> b;
    void bytes(const void* p, size_t n) { const uint8_t* q = static_cast<const uint8_t*>(p); b.insert(b.end(), q, q + n); }
    template <typename T> void put(const T& v) { bytes(&v, sizeof(T)); }
    template <typename T> void vec(const std::vector<T>& v) { put<uint64_t>(v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
};
struct SessReader {
    const uint8_t* p; size_t n, at = 0; bool ok = true;
    SessReader(const std::vector<uint8_t>& v) : p(v.data()), n(v.size()) {}
    void bytes(void* out, size_t k) {
        if (!ok || k > n - at) { ok = false; memset(out, 0, k); return; }
        memcpy(out, p + at, k); at += k;
    }
    template <typename T> T get() { T v; bytes(&v, sizeof(T)); return v; }
    template <typename T> void vec(std::vector<T>& v) {
        const uint64_t k = get<uint64_t>();
        if (!ok || k > (n - at) / sizeof(T)) { ok = false; v.clear(); return; }
        v.resize((size_t)k);
        if (k) bytes(v.data(), (size_t)k * sizeof(T));
    }
};

// one section of a save / a digest: host bytes, a block of device memory, or a model's live surfels
struct SessSection {
    std::string name; int owner = -1;
    std::vector<uint8_t> host;                       // host sections
    const void* dev = nullptr; uint64_t bytes = 0;   // device blocks (bytes 0: absent, digest 0)
    ModelState* surfels = nullptr; int n = 0;        // "surfels": the model and its live count
    bool on_device = false;
    uint64_t offset = 0, digest = 0;
};

uint64_t up256(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }

}  // namespace

// Staging of a save / load / digest, allocated on the first call and freed by mf_destroy: nothing of it is shared with the frame path
struct SessionScratch {
    int* d_offs = nullptr;                           // run offsets of the buffer being walked (+ its live count behind them)
    int* d_total = nullptr;                          // [256] live counts, one per model
    unsigned long long* d_words = nullptr; size_t words_cap = 0;
    float4* d_stage[2] = {nullptr, nullptr};         // kSessionChunk records each
    uint8_t* h_pin[2] = {nullptr, nullptr};          // pinned, the same size
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~SessionScratch() {
        for (void* q : {(void*)d_offs, (void*)d_total, (void*)d_words, (void*)d_stage[0], (void*)d_stage[1]})
            if (q) (void)hipFree(q);
        for (int i = 0; i < 2; ++i) {
            if (h_pin[i]) (void)hipHostFree(h_pin[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
};
static void session_free(SessionScratch* s) { delete s; }
static constexpr size_t kSessionStageBytes = (size_t)kSessionChunk * 48;
static constexpr size_t kSessionWords = MF_STATE_CONTEXT_SECTIONS + 256 * MF_STATE_MODEL_SECTIONS + 256 * 6;   // (+ the pool's pyramids)

static int session_scratch(mf_ctx* c, bool staging) {
    if (!c->session) c->session = new SessionScratch();
    SessionScratch& s = *c->session;
    if (!s.d_offs) MF_HIP(c, hipMalloc(&s.d_offs, (run_table_runs((long)c->cap_max, (long)c->P) + 2) * sizeof(int)));
    if (!s.d_total) MF_HIP(c, hipMalloc(&s.d_total, 256 * sizeof(int)));
    if (!s.d_words) { MF_HIP(c, hipMalloc(&s.d_words, kSessionWords * sizeof(unsigned long long))); s.words_cap = kSessionWords; }
    for (int i = 0; i < 2 && staging; ++i) {
        if (!s.d_stage[i]) MF_HIP(c, hipMalloc(&s.d_stage[i], kSessionStageBytes));
        if (!s.h_pin[i]) MF_HIP(c, hipHostMalloc(&s.h_pin[i], kSessionStageBytes));
        if (!s.ev[i]) MF_HIP(c, hipEventCreateWithFlags(&s.ev[i], hipEventDisableTiming));
    }
    return MF_OK;
}
static int session_quiesce(mf_ctx* c) {   // every stream of the context is idle: the buffers are as the last call left them
    MF_HIP(c, hipStreamSynchronize(c->stream));
    if (c->stream_obj) MF_HIP(c, hipStreamSynchronize(c->stream_obj));
    if (c->stream_in) MF_HIP(c, hipStreamSynchronize(c->stream_in));
    return MF_OK;
}

// the last staged frame lies in the context's own input blocks (mf_process_frame, mf_stage_frame): which one, or -1 (the caller's memory, or none)
static int staged_slot(const mf_ctx* c) {
    for (int i = 0; i < 2; ++i)
        if (c->cur_rgb && c->cur_rgb == c->d_in_rgb[i] && c->cur_depth == c->d_in_depth[i]) return i;
    return -1;
}
static size_t used_log_entries(const mf_ctx* c, const ModelState& m) {
    if (!m.d_poselog) return 0;
    return std::min(m.log_ts.size(), (size_t)c->cfg.pose_log_capacity);
}

// The device-resident sections of the context and its models, in mf_state_digest's order.  Read-only.  Live counts: s.d_total[model] (device) and,
// with host_counts, on the host (one synchronisation).  with_pool: behind them the model-side pyramids of the preallocated models, owner = models in the
// list + position in the pool -- a spawn takes its model from the pool's front, and until the model is tracked its pyramid planes (debug taps
// "vmap_g" / "nmap_g") still hold what the pool member's last tracking step left
static void session_pyramid_sections(const mf_ctx* c, const ModelState& m, int owner, std::vector<SessSection>& out) {
    for (int i = 0; i < 3; ++i)
        for (int n = 0; n < 2; ++n) {
            SessSection q; q.name = kModelSections[10 + 2 * i + n]; q.owner = owner; q.dev = n ? m.d_nmap_g[i] : m.d_vmap_g[i];
            q.bytes = (uint64_t)(c->W >> i) * (c->H >> i) * 3 * sizeof(float); q.on_device = true;
            out.push_back(std::move(q));
        }
}
static int session_device_sections(mf_ctx* c, std::vector<SessSection>& out, bool host_counts, bool with_pool) {
    SessionScratch& s = *c->session;
    const size_t P = (size_t)c->P;
    auto add = [&](const char* name, int owner, const void* p, uint64_t bytes) {
        SessSection q; q.name = name; q.owner = owner; q.dev = p; q.bytes = p ? bytes : 0; q.on_device = true;
        out.push_back(std::move(q));
    };
    int k = 0;
    add(kCtxSections[k++], -1, c->d_mask_tex, P);
    add(kCtxSections[k++], -1, c->labels ? c->labels->ignoreMap : nullptr, P);
    for (int b = 0; b < 3; ++b) add(kCtxSections[k++], -1, c->d_depthF[b], P * sizeof(float));
    for (int set = 0; set < 2; ++set)
        for (int i = 0; i < 3; ++i) add(kCtxSections[k++], -1, c->d_gray[set][i], (size_t)(c->W >> i) * (c->H >> i));
    const int slot = staged_slot(c);
    add(kCtxSections[k++], -1, slot >= 0 ? c->d_in_rgb[slot] : nullptr, P * 3);
    add(kCtxSections[k++], -1, slot >= 0 ? (const void*)c->d_in_depth[slot] : nullptr, P * sizeof(float));
    add(kCtxSections[k++], -1, slot >= 0 ? c->d_in_mask[slot] : nullptr, P);
    if (c->models.size() > 256) { c->err = "session: more than 256 models"; return MF_ESTATE; }
    for (size_t i = 0; i < c->models.size(); ++i) {
        ModelState& m = *c->models[i];
        // the live count of the buffer as it stands, dense or run-structured (the offsets themselves are recomputed where the buffer is walked)
        launch_run_offsets(m.surf[m.cur], m.d_frame, s.d_offs, s.d_total + i, c->stream);
        SessSection q; q.name = kModelSections[0]; q.owner = (int)i; q.surfels = &m; q.on_device = true;
        out.push_back(std::move(q));
        add(kModelSections[1], (int)i, m.d_pose, sizeof(PoseDev));
        add(kModelSections[2], (int)i, m.d_frame, sizeof(FrameDev));
        add(kModelSections[3], (int)i, m.d_predV, P * sizeof(float4));
        add(kModelSections[4], (int)i, m.d_predN, P * sizeof(float4));
        add(kModelSections[5], (int)i, m.d_predImage, P * sizeof(uchar4));
        add(kModelSections[6], (int)i, m.d_predTime, P * sizeof(uint16_t));
        add(kModelSections[7], (int)i, m.d_predGray, P);
        add(kModelSections[8], (int)i, m.d_fillGray, P);
        add(kModelSections[9], (int)i, m.d_poselog, used_log_entries(c, m) * 8 * sizeof(float));
        session_pyramid_sections(c, m, (int)i, out);
    }
    for (size_t j = 0; j < c->pool.size() && with_pool; ++j) session_pyramid_sections(c, *c->pool[j], (int)(c->models.size() + j), out);
    if (host_counts && !c->models.empty()) {
        std::vector<int> totals(c->models.size());
        MF_HIP(c, hipMemcpyAsync(totals.data(), s.d_total, totals.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        MF_HIP(c, hipStreamSynchronize(c->stream));
        for (SessSection& q : out)
            if (q.surfels) { q.n = std::max(0, std::min(totals[q.owner], q.surfels->cap)); q.bytes = (uint64_t)q.n * 48u; }
    }
    return MF_OK;
}
// their digests, on the device: words[i] for sections[i] (one synchronisation)
static int session_device_digests(mf_ctx* c, std::vector<SessSection>& secs) {
    SessionScratch& s = *c->session;
    if (secs.size() > s.words_cap) { c->err = "session: too many sections"; return MF_ESTATE; }
    MF_HIP(c, hipMemsetAsync(s.d_words, 0, secs.size() * sizeof(unsigned long long), c->stream));
    for (size_t i = 0; i < secs.size(); ++i) {
        SessSection& q = secs[i];
        if (q.surfels) {
            ModelState& m = *q.surfels;
            launch_run_offsets(m.surf[m.cur], m.d_frame, s.d_offs, nullptr, c->stream);
            launch_state_digest_surfels(m.surf[m.cur], m.d_frame, s.d_offs, s.d_total + q.owner, *m.h_count, s.d_words + i, c->stream);
        } else if (q.bytes) {
            launch_state_digest(q.dev, q.bytes, 0, s.d_words + i, c->stream);
        }
    }
    std::vector<unsigned long long> w(secs.size());
    if (!w.empty()) MF_HIP(c, hipMemcpyAsync(w.data(), s.d_words, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    MF_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < secs.size(); ++i) secs[i].digest = (uint64_t)w[i];
    int rc = check_launch(c);
    return rc;
}

extern "C" const char* mf_state_section_name(int32_t i) {
    if (i < 0 || i >= MF_STATE_CONTEXT_SECTIONS + MF_STATE_MODEL_SECTIONS) return nullptr;
    return i < MF_STATE_CONTEXT_SECTIONS ? kCtxSections[i] : kModelSections[i - MF_STATE_CONTEXT_SECTIONS];
}

extern "C" int mf_state_digest(mf_ctx* c, uint64_t* out, int32_t capacity, int32_t* n) {
    settle(c);
    if (!c || !out || !n) return MF_EINVAL;
    const size_t words = MF_STATE_CONTEXT_SECTIONS + c->models.size() * MF_STATE_MODEL_SECTIONS;
    *n = (int32_t)words;
    if ((size_t)std::max(capacity, 0) < words) { c->err = "mf_state_digest: capacity is smaller than the number of sections"; return MF_EINVAL; }
    int rc = session_quiesce(c);
    if (rc == MF_OK) rc = session_scratch(c, false);
    std::vector<SessSection> secs;
    if (rc == MF_OK) rc = session_device_sections(c, secs, false, false);
    if (rc == MF_OK) rc = session_device_digests(c, secs);
    if (rc != MF_OK) return rc;
    for (size_t i = 0; i < words; ++i) out[i] = secs[i].digest;
    return MF_OK;
}

// tooling (tools/session_timing.py): GPU milliseconds, between HIP events, of k_session_pack over the model's whole live buffer (chunk by chunk into
// the staging block, no copy) and of k_state_digest_surfels over it; *surfels: its live count.  Read-only like a save.
extern "C" int mf_k_session_timing(mf_ctx* c, int32_t model, float* ms2, uint32_t* surfels) {
    settle(c);
    ModelState* m = model_at(c, model);
    if (!m || !ms2 || !surfels) return MF_EINVAL;
    int rc = session_quiesce(c);
    if (rc == MF_OK) rc = session_scratch(c, true);
    if (rc != MF_OK) return rc;
    SessionScratch& s = *c->session;
    hipStream_t st = c->stream;
    const Surfels& sf = m->surf[m->cur];
    int total = 0;
    launch_run_offsets(sf, m->d_frame, s.d_offs, s.d_total, st);
    MF_HIP(c, hipMemcpyAsync(&total, s.d_total, sizeof(int), hipMemcpyDeviceToHost, st));
    MF_HIP(c, hipStreamSynchronize(st));
    const int n = std::max(0, std::min(total, m->cap));
    *surfels = (uint32_t)n;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    for (hipEvent_t& e : ev) MF_HIP(c, hipEventCreate(&e));
    MF_HIP(c, hipMemsetAsync(s.d_words, 0, sizeof(unsigned long long), st));
    (void)hipEventRecord(ev[0], st);
    for (int first = 0; first < n; first += kSessionChunk)
        launch_session_pack(sf, m->d_frame, s.d_offs, first, std::min(kSessionChunk, n - first), s.d_stage[(first / kSessionChunk) & 1], st);
    (void)hipEventRecord(ev[1], st);
    launch_state_digest_surfels(sf, m->d_frame, s.d_offs, s.d_total, n, s.d_words, st);
    (void)hipEventRecord(ev[2], st);
    const bool ok = hipStreamSynchronize(st) == hipSuccess && hipEventElapsedTime(&ms2[0], ev[0], ev[1]) == hipSuccess &&
                    hipEventElapsedTime(&ms2[1], ev[1], ev[2]) == hipSuccess;
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    if (!ok) { c->err = "mf_k_session_timing: the timed launches failed"; (void)hipGetLastError(); return MF_EHIP; }
    return check_launch(c);
}

// ---- the host sections ----
static void session_host_sections(mf_ctx* c, const void* user, uint64_t user_bytes, const std::vector<std::vector<float>>& retired_p,
                                  std::vector<SessSection>& out) {
    auto add = [&](const char* name, int owner, SessWriter& w) {
        SessSection q; q.name = name; q.owner = owner; q.host = std::move(w.b); q.bytes = q.host.size();
        out.push_back(std::move(q));
    };
    { SessWriter w; w.put(c->cfg); add("config", -1, w); }
    {   // every read-write row of the table, by key
        SessWriter w;
        std::vector<std::pair<std::string, double>> rows;
        for (const ParamRow& p : kParamTable) {
            if (p.access != kReadWrite) continue;
            double v = 0;
            if (p.get) { if (p.get(c, p, &v) != MF_OK) continue; }
            else {
                const char* at = param_home(c, p);
                v = p.type == kFlag ? (*reinterpret_cast<const bool*>(at) ? 1 : 0) : p.type == kInt ? (double)*reinterpret_cast<const int32_t*>(at)
                                                                                                   : (double)*reinterpret_cast<const float*>(at);
            }
            rows.emplace_back(p.key, v);
        }
        w.put<uint32_t>((uint32_t)rows.size());
        for (auto& r : rows) { w.put<uint32_t>((uint32_t)r.first.size()); w.bytes(r.first.data(), r.first.size()); w.put<double>(r.second); }
        add("params", -1, w);
    }
    {
        SessWriter w;
        w.put<uint32_t>((uint32_t)sizeof(SegParams)); w.put(c->seg);
        w.put<int64_t>(c->frame_no); w.put<int32_t>(c->host_tick); w.put<uint8_t>(c->map_ready); w.put<uint8_t>(c->tracked_once);
        w.put<int32_t>(c->nextID); w.put<int32_t>(c->spawnOffset); w.put<int32_t>(c->lastF);
        w.put<int64_t>(c->gray_frame[0]); w.put<int64_t>(c->gray_frame[1]); w.put<int64_t>(c->deriv_frame); w.put<int64_t>(c->bg_fused_frame);
        w.put<uint8_t>(c->iclean_is_tap16); w.put<uint8_t>(staged_slot(c) >= 0);
        // the read-only counters a continued run goes on counting
        int fixups = 0;
        (void)hipMemcpy(&fixups, c->d_pyramid_fixups, sizeof(int), hipMemcpyDeviceToHost);
        w.put<int32_t>(c->densify_count); w.put<int64_t>(c->deferred_frames); w.put<int64_t>(c->fused_head_frames); w.put<int32_t>(fixups);
        w.put<uint32_t>((uint32_t)c->pool.size());
        w.vec(c->mask_classes); w.vec(c->trackable);
        add("context", -1, w);
    }
    { SessWriter w; w.bytes(c->ignoreMap.data(), c->ignoreMap.size()); add("ignore_map_host", -1, w); }
    {
        SessWriter w;
        w.put<uint32_t>((uint32_t)c->retired.size());
        for (size_t i = 0; i < c->retired.size(); ++i) { w.put<int32_t>(c->retired[i].id); w.vec(c->retired[i].ts); w.vec(retired_p[i]); }
        add("retired", -1, w);
    }
    for (size_t i = 0; i < c->models.size(); ++i) {
        const ModelState& m = *c->models[i];
        SessWriter w;
        w.put<int32_t>(m.id); w.put<int32_t>(m.classID); w.put<uint8_t>(m.isStatic); w.put<uint8_t>(m.allowFillIn); w.put<uint8_t>(m.pred_gray_valid);
        w.put<uint8_t>(m.table_valid);
        w.put<uint32_t>(m.age); w.put<float>(m.confThr); w.put<float>(m.maxDepth); w.put<int32_t>(m.cap);
        w.put(*m.h_pose); w.put(*m.h_frame);
        w.vec(m.log_ts);
        add("model", (int)i, w);
    }
    { SessWriter w; if (user_bytes) w.bytes(user, (size_t)user_bytes); add("user", -1, w); }
    if (!c->inactive.empty()) {   // the kept maps of dropped models, last: a file of a context without any has the sections it always had
        SessWriter w;
        w.put<uint32_t>((uint32_t)c->inactive.size());
        for (const mf_ctx::Inactive& a : c->inactive) {
            w.put<uint32_t>((uint32_t)sizeof(mf_inactive_info_t)); w.put(a.info);
            std::vector<float> rec((size_t)a.info.surfels * 12);
            if (!rec.empty()) (void)hipMemcpy(rec.data(), a.d_rec, rec.size() * sizeof(float), hipMemcpyDeviceToHost);
            w.vec(rec);
        }
        add("inactive", -1, w);
    }
}

extern "C" int mf_session_save(mf_ctx* c, const char* path, const void* user, uint64_t user_bytes) {
    settle(c);
    if (!c || !path || (!user && user_bytes)) return MF_EINVAL;
    int rc = session_quiesce(c);
    if (rc == MF_OK) rc = session_scratch(c, true);
    if (rc != MF_OK) return rc;
    SessionScratch& s = *c->session;
    hipStream_t st = c->stream;
    std::vector<SessSection> secs;
    rc = session_device_sections(c, secs, true, true);
    if (rc == MF_OK) rc = session_device_digests(c, secs);
    if (rc != MF_OK) return rc;
    // the retired pose logs: those still in the device arena are read back for the file; the arena and the records stay as they are
    std::vector<std::vector<float>> retired_p(c->retired.size());
    for (size_t i = 0; i < c->retired.size(); ++i) {
        const mf_ctx::RetiredLog& r = c->retired[i];
        if (!r.in_arena) { retired_p[i] = r.p; continue; }
        std::vector<float> raw(r.n * 8);
        if (r.n) MF_HIP(c, hipMemcpy(raw.data(), c->d_retired + r.arena_off * 8, r.n * 8 * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < r.n; ++e) retired_p[i].insert(retired_p[i].end(), raw.data() + e * 8, raw.data() + e * 8 + 7);
    }
    session_host_sections(c, user, user_bytes, retired_p, secs);
    SessionHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kSessionMagic, 8);
    h.version = MF_SESSION_VERSION; h.pose_bytes = sizeof(PoseDev); h.frame_bytes = sizeof(FrameDev); h.run = kRun;
    h.width = c->W; h.height = c->H; h.n_models = (int32_t)c->models.size(); h.tick = c->host_tick; h.user_bytes = user_bytes;
    h.n_sections = (uint32_t)secs.size(); h.config_bytes = sizeof(mf_config); h.frames = c->frame_no;
    std::vector<SessionEntry> table(secs.size());
    uint64_t at = up256(sizeof(h) + table.size() * sizeof(SessionEntry));
    for (size_t i = 0; i < secs.size(); ++i) {
        SessSection& q = secs[i];
        if (!q.on_device) q.digest = state_digest_host(q.host.data(), q.bytes);
        q.offset = at;
        at = up256(at + q.bytes);
        SessionEntry& e = table[i];
        memset(&e, 0, sizeof(e));
        snprintf(e.name, sizeof(e.name), "%s", q.name.c_str());
        e.owner = q.owner; e.offset = q.offset; e.bytes = q.bytes; e.digest = q.digest;
    }
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { c->err = "mf_session_save: cannot write " + tmp; return MF_EINVAL; }
    uint64_t pos = 0;
    bool ok = true;
    auto put = [&](const void* p, size_t n) { if (ok && n) ok = fwrite(p, 1, n, f) == n; pos += n; };
    auto pad_to = [&](uint64_t off) { static const uint8_t zeros[256] = {}; while (ok && pos < off) put(zeros, (size_t)std::min<uint64_t>(256, off - pos)); };
    auto fail = [&](int code, const std::string& why) { fclose(f); remove(tmp.c_str()); c->err = why; return code; };
    put(&h, sizeof(h));
    put(table.data(), table.size() * sizeof(SessionEntry));
    for (SessSection& q : secs) {
        pad_to(q.offset);
        if (!q.on_device) { put(q.host.data(), q.host.size()); continue; }
        if (q.surfels) {
            // chunk k: one pack launch, then its copy into pinned buffer k & 1; the file write of chunk k - 1 runs under that copy
            ModelState& m = *q.surfels;
            launch_run_offsets(m.surf[m.cur], m.d_frame, s.d_offs, nullptr, st);
            const int chunks = (q.n + kSessionChunk - 1) / kSessionChunk;
            for (int k = 0; k <= chunks; ++k) {
                if (k < chunks) {
                    const int first = k * kSessionChunk, n = std::min(kSessionChunk, q.n - first);
                    launch_session_pack(m.surf[m.cur], m.d_frame, s.d_offs, first, n, s.d_stage[k & 1], st);
                    if (hipMemcpyAsync(s.h_pin[k & 1], s.d_stage[k & 1], (size_t)n * 48, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipEventRecord(s.ev[k & 1], st) != hipSuccess)
                        return fail(MF_EHIP, "mf_session_save: copying a surfel chunk failed");
                }
                if (k > 0) {
                    const int first = (k - 1) * kSessionChunk, n = std::min(kSessionChunk, q.n - first);
                    if (hipEventSynchronize(s.ev[(k - 1) & 1]) != hipSuccess) return fail(MF_EHIP, "mf_session_save: a surfel chunk did not arrive");
                    put(s.h_pin[(k - 1) & 1], (size_t)n * 48);
                }
            }
            continue;
        }
        for (uint64_t done = 0; done < q.bytes; done += kSessionStageBytes) {
            const size_t n = (size_t)std::min<uint64_t>(kSessionStageBytes, q.bytes - done);
            if (hipMemcpyAsync(s.h_pin[0], static_cast<const uint8_t*>(q.dev) + done, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return fail(MF_EHIP, "mf_session_save: copying section " + q.name + " failed");
            put(s.h_pin[0], n);
        }
    }
    pad_to(at);
    if (!ok) return fail(MF_EINVAL, "mf_session_save: writing " + tmp + " failed");
    if (fclose(f) != 0) { remove(tmp.c_str()); c->err = "mf_session_save: writing " + tmp + " failed"; return MF_EINVAL; }
    if (rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); c->err = std::string("mf_session_save: cannot move the file to ") + path; return MF_EINVAL; }
    return check_launch(c);
}

// ---- reading ----
static int session_refuse(const std::string& why) { return cloud_fail("mf_session", why.c_str(), MF_EINVAL); }
// header and section table of an open file, checked against this build and the file's size
static int session_read_index(FILE* f, SessionHeader& h, std::vector<SessionEntry>& table, uint64_t& file_bytes) {
    if (fseek(f, 0, SEEK_END) != 0) return session_refuse("cannot seek");
    const long end = ftell(f);
    if (end < 0) return session_refuse("cannot seek");
    file_bytes = (uint64_t)end;
    rewind(f);
    if (file_bytes < sizeof(h) || fread(&h, 1, sizeof(h), f) != sizeof(h)) return session_refuse("the file is shorter than a session header");
    if (memcmp(h.magic, kSessionMagic, 8) != 0) return session_refuse("not a session file (wrong magic)");
    if (h.version != MF_SESSION_VERSION) return session_refuse("format version " + std::to_string(h.version) + ", this build reads " + std::to_string(MF_SESSION_VERSION));
    if (h.pose_bytes != sizeof(PoseDev) || h.frame_bytes != sizeof(FrameDev) || h.config_bytes != sizeof(mf_config) || h.run != (uint32_t)kRun)
        return session_refuse("written by another build of the library: sizeof(PoseDev) / sizeof(FrameDev) / sizeof(mf_config) / run length are " +
                              std::to_string(h.pose_bytes) + " / " + std::to_string(h.frame_bytes) + " / " + std::to_string(h.config_bytes) + " / " + std::to_string(h.run) +
                              ", this build has " + std::to_string(sizeof(PoseDev)) + " / " + std::to_string(sizeof(FrameDev)) + " / " + std::to_string(sizeof(mf_config)) +
                              " / " + std::to_string(kRun));
    if (h.n_sections > 65536 || h.n_models < 0 || h.n_models > 256 || h.width <= 0 || h.height <= 0) return session_refuse("implausible header");
    const uint64_t table_end = sizeof(h) + (uint64_t)h.n_sections * sizeof(SessionEntry);
    if (table_end > file_bytes) return session_refuse("the file is short: the section table ends at byte " + std::to_string(table_end) + " of " + std::to_string(file_bytes));
    table.resize(h.n_sections);
    if (h.n_sections && fread(table.data(), sizeof(SessionEntry), h.n_sections, f) != h.n_sections) return session_refuse("cannot read the section table");
    for (SessionEntry& e : table) {
        e.name[sizeof(e.name) - 1] = 0;
        if (e.offset < table_end || (e.offset & 255u) || e.bytes > file_bytes || e.offset > file_bytes - e.bytes)
            return session_refuse(std::string("the file is short: section ") + e.name + " lies outside it");
    }
    return MF_OK;
}
static const SessionEntry* session_find(const std::vector<SessionEntry>& table, const char* name, int owner) {
    for (const SessionEntry& e : table)
        if (e.owner == owner && !strcmp(e.name, name)) return &e;
    return nullptr;
}
// a host section's bytes, digest checked
static int session_read_host(FILE* f, const std::vector<SessionEntry>& table, const char* name, int owner, std::vector<uint8_t>& out) {
    const SessionEntry* e = session_find(table, name, owner);
    if (!e) return session_refuse(std::string("section ") + name + " is missing");
    if (e->bytes > ((uint64_t)1 << 31)) return session_refuse(std::string("section ") + name + " is implausibly large");
    out.resize((size_t)e->bytes);
    if (fseek(f, (long)e->offset, SEEK_SET) != 0 || (e->bytes && fread(out.data(), 1, out.size(), f) != out.size()))
        return session_refuse(std::string("cannot read section ") + name);
    if (state_digest_host(out.data(), out.size()) != e->digest) return session_refuse(std::string("section ") + name + ": the digest does not match its bytes");
    return MF_OK;
}

extern "C" int mf_session_info(const char* path, mf_session_info_t* out, void* user, uint64_t user_capacity, uint64_t* user_bytes) {
    if (!path || !out) return MF_EINVAL;
    FILE* f = fopen(path, "rb");
    if (!f) return session_refuse(std::string("cannot open ") + path);
    SessionHeader h; std::vector<SessionEntry> table; uint64_t file_bytes = 0;
    int rc = session_read_index(f, h, table, file_bytes);
    std::vector<uint8_t> blob;
    if (rc == MF_OK) rc = session_read_host(f, table, "user", -1, blob);
    fclose(f);
    if (rc != MF_OK) return rc;
    if (blob.size() != h.user_bytes) return session_refuse("the user blob's size differs from the header's");
    memset(out, 0, sizeof(*out));
    out->version = h.version; out->width = h.width; out->height = h.height; out->n_models = h.n_models; out->tick = h.tick; out->n_sections = h.n_sections;
    out->frames = h.frames; out->user_bytes = h.user_bytes; out->file_bytes = file_bytes;
    out->pose_bytes = h.pose_bytes; out->frame_bytes = h.frame_bytes; out->run = h.run; out->config_bytes = h.config_bytes;
    if (user_bytes) *user_bytes = blob.size();
    if (user && user_capacity && !blob.empty()) memcpy(user, blob.data(), (size_t)std::min<uint64_t>(user_capacity, blob.size()));
    return MF_OK;
}

static __global__ void k_session_dense_count(FrameDev* f, int count) {   // the loaded buffer: dense, slots [0, count), no table yet
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    f->count = count; f->countNext = count; f->phys = count; f->runs = 0; f->runsNext = 0; f->first = 0; f->first_run = 0;
}

// a device block's bytes from the file into dst (bytes 0: the section is absent and dst keeps its contents), its digest accumulated into *word
static int session_load_block(mf_ctx* c, FILE* f, const SessionEntry& e, void* dst, uint64_t expect, unsigned long long* word) {
    SessionScratch& s = *c->session;
    if (e.bytes == 0) return MF_OK;
    if (!dst || e.bytes != expect) return session_refuse(std::string("section ") + e.name + " has " + std::to_string(e.bytes) + " bytes, this context holds " + std::to_string(dst ? expect : 0));
    if (fseek(f, (long)e.offset, SEEK_SET) != 0) return session_refuse(std::string("cannot read section ") + e.name);
    for (uint64_t done = 0; done < e.bytes; done += kSessionStageBytes) {
        const size_t n = (size_t)std::min<uint64_t>(kSessionStageBytes, e.bytes - done);
        if (fread(s.h_pin[0], 1, n, f) != n) return session_refuse(std::string("cannot read section ") + e.name);
        MF_HIP(c, hipMemcpyAsync(static_cast<uint8_t*>(dst) + done, s.h_pin[0], n, hipMemcpyHostToDevice, c->stream));
        MF_HIP(c, hipStreamSynchronize(c->stream));
    }
    launch_state_digest(dst, e.bytes, 0, word, c->stream);
    return MF_OK;
}

extern "C" int mf_session_load(const char* path, int32_t device, mf_ctx** out) {
    if (!path || !out) return MF_EINVAL;
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return session_refuse(std::string("cannot open ") + path);
    mf_ctx* c = nullptr;
    auto fail = [&](int code) {             // the reason is in mf_last_error(NULL) already (session_refuse)
        if (c) mf_destroy(c);
        fclose(f);
        return code;
    };
    auto fail_ctx = [&](int code) {         // ... or in the half-built context, which it has to outlive
        cloud_fail("mf_session_load", c->err.c_str(), code);
        return fail(code);
    };
#define LOAD_HIP(call) do { if ((call) != hipSuccess) { c->err = #call " failed"; (void)hipGetLastError(); return fail_ctx(MF_EHIP); } } while (0)
    SessionHeader h; std::vector<SessionEntry> table; uint64_t file_bytes = 0;
    int rc = session_read_index(f, h, table, file_bytes);
    if (rc != MF_OK) return fail(rc);
    std::vector<uint8_t> b_cfg, b_params, b_ctx, b_ignore, b_retired;
    if ((rc = session_read_host(f, table, "config", -1, b_cfg)) != MF_OK || (rc = session_read_host(f, table, "params", -1, b_params)) != MF_OK ||
        (rc = session_read_host(f, table, "context", -1, b_ctx)) != MF_OK || (rc = session_read_host(f, table, "ignore_map_host", -1, b_ignore)) != MF_OK ||
        (rc = session_read_host(f, table, "retired", -1, b_retired)) != MF_OK)
        return fail(rc);
    std::vector<std::vector<uint8_t>> b_models((size_t)h.n_models);
    for (int i = 0; i < h.n_models; ++i)
        if ((rc = session_read_host(f, table, "model", i, b_models[i])) != MF_OK) return fail(rc);
    if (b_cfg.size() != sizeof(mf_config) || h.n_models < 1) return fail(session_refuse("section config: wrong size"));
    mf_config cfg;
    memcpy(&cfg, b_cfg.data(), sizeof(cfg));
    if (cfg.width != h.width || cfg.height != h.height) return fail(session_refuse("section config disagrees with the header"));
    if (device >= 0) cfg.device = device;
    rc = mf_create(&cfg, &c);
    if (rc != MF_OK) { c = nullptr; cloud_fail("mf_session_load", "mf_create with the saved configuration failed", rc); return fail(rc); }
    if ((rc = session_scratch(c, true)) != MF_OK) return fail_ctx(rc);
    SessionScratch& s = *c->session;
    hipStream_t st = c->stream;
    const size_t P = (size_t)c->P;
    {   // every read-write row, through its setter
        SessReader r(b_params);
        const uint32_t rows = r.get<uint32_t>();
        for (uint32_t i = 0; i < rows && r.ok; ++i) {
            const uint32_t len = r.get<uint32_t>();
            if (!r.ok || len > 256) { r.ok = false; break; }
            std::string key(len, '\0');
            r.bytes(&key[0], len);
            const double v = r.get<double>();
            if (!r.ok) break;
            const ParamRow* p = find_param(key.c_str());
            if (!p || p->access != kReadWrite) return fail(session_refuse("section params: unknown key " + key));
            if ((rc = mf_set_param(c, key.c_str(), v)) != MF_OK) return fail_ctx(rc);
        }
        if (!r.ok) return fail(session_refuse("section params is malformed"));
    }
    uint32_t pool = 0; bool staged = false; int fixups = 0;
    {
        SessReader r(b_ctx);
        if (r.get<uint32_t>() != sizeof(SegParams)) return fail(session_refuse("written by another build of the library: sizeof(SegParams) differs"));
        c->seg = r.get<SegParams>();
        c->frame_no = (long)r.get<int64_t>(); c->host_tick = r.get<int32_t>(); c->map_ready = r.get<uint8_t>() != 0; c->tracked_once = r.get<uint8_t>() != 0;
        c->nextID = r.get<int32_t>(); c->spawnOffset = r.get<int32_t>(); c->lastF = r.get<int32_t>();
        c->gray_frame[0] = (long)r.get<int64_t>(); c->gray_frame[1] = (long)r.get<int64_t>(); c->deriv_frame = (long)r.get<int64_t>();
        c->bg_fused_frame = (long)r.get<int64_t>();
        c->iclean_is_tap16 = r.get<uint8_t>() != 0; staged = r.get<uint8_t>() != 0;
        c->densify_count = r.get<int32_t>(); c->deferred_frames = (long)r.get<int64_t>(); c->fused_head_frames = (long)r.get<int64_t>(); fixups = r.get<int32_t>();
        pool = r.get<uint32_t>();
        r.vec(c->mask_classes); r.vec(c->trackable);
        if (!r.ok || c->lastF < 0 || c->lastF > 2 || c->frame_no < 0 || c->host_tick < 1 || pool > 256) return fail(session_refuse("section context is malformed"));
        // the derivative images belong to one frame and are not saved: the next frame with a photometric term computes its own
        c->deriv_frame = -1;
    }
    LOAD_HIP((hipMemcpy(c->d_pyramid_fixups, &fixups, sizeof(int), hipMemcpyHostToDevice)));
    if (b_ignore.size() != P) return fail(session_refuse("section ignore_map_host: wrong size"));
    c->ignoreMap.assign(b_ignore.begin(), b_ignore.end());
    {
        SessReader r(b_retired);
        const uint32_t n = r.get<uint32_t>();
        for (uint32_t i = 0; i < n && r.ok; ++i) {
            mf_ctx::RetiredLog q;
            q.id = r.get<int32_t>(); r.vec(q.ts); r.vec(q.p);
            if (!r.ok || q.p.size() != q.ts.size() * 7) { r.ok = false; break; }
            q.n = q.ts.size();
            c->retired.push_back(std::move(q));
        }
        if (!r.ok) return fail(session_refuse("section retired is malformed"));
    }
    if (session_find(table, "inactive", -1)) {   // (optional: written only for a list that is not empty)
        std::vector<uint8_t> b_inactive;
        if ((rc = session_read_host(f, table, "inactive", -1, b_inactive)) != MF_OK) return fail(rc);
        SessReader r(b_inactive);
        const uint32_t n = r.get<uint32_t>();
        for (uint32_t i = 0; i < n && r.ok; ++i) {
            mf_ctx::Inactive a;
            if (r.get<uint32_t>() != sizeof(mf_inactive_info_t)) { r.ok = false; break; }
            a.info = r.get<mf_inactive_info_t>();
            std::vector<float> rec;
            r.vec(rec);
            if (!r.ok || rec.size() != (size_t)a.info.surfels * 12) { r.ok = false; break; }
            if (!rec.empty()) {
                LOAD_HIP((hipMalloc(&a.d_rec, rec.size() * sizeof(float))));
                c->inactive.push_back(a);   // (owned by the context from here on: a failure below frees it with the context)
                LOAD_HIP((hipMemcpy(a.d_rec, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice)));
            } else c->inactive.push_back(a);
        }
        if (!r.ok) return fail(session_refuse("section inactive is malformed"));
    }
    // the model list in order, with the saved ids and classes
    const int cap_obj = surfel_capacity(c->cfg.num_osurfels);
    std::vector<uint8_t> had_table((size_t)h.n_models);
    for (int i = 0; i < h.n_models; ++i) {
        SessReader r(b_models[i]);
        const int32_t id = r.get<int32_t>(), classID = r.get<int32_t>();
        const bool isStatic = r.get<uint8_t>() != 0, allowFillIn = r.get<uint8_t>() != 0, gray_valid = r.get<uint8_t>() != 0;
        had_table[i] = r.get<uint8_t>();
        const uint32_t age = r.get<uint32_t>(); const float confThr = r.get<float>(), maxDepth = r.get<float>(); const int32_t cap = r.get<int32_t>();
        if (!r.ok || allowFillIn != (i == 0)) return fail(session_refuse("section model is malformed"));
        if (i > 0) {
            std::unique_ptr<ModelState> nm;
            if ((rc = create_model(c, id, c->cfg.conf_object, false, cap_obj, nm)) != MF_OK) return fail_ctx(rc);
            c->models.push_back(std::move(nm));
        }
        ModelState& m = *c->models[i];
        if (cap != m.cap) return fail(session_refuse("section model: the surfel capacity differs from the configuration's"));
        m.id = id; m.classID = classID; m.isStatic = isStatic; m.pred_gray_valid = gray_valid; m.age = age; m.confThr = confThr; m.maxDepth = maxDepth;
        *m.h_pose = r.get<PoseDev>(); *m.h_frame = r.get<FrameDev>();
        r.vec(m.log_ts);
        if (!r.ok) return fail(session_refuse("section model is malformed"));
    }
    // (as spawn_object: the private scratch of the batched object passes is allocated outside a frame; a failure only switches them off)
    if (c->sw.batch_objects && c->models.size() >= 3)
        for (size_t i = 1; i < c->models.size(); ++i)
            if (ensure_obj_scratch(c, *c->models[i]) != MF_OK) { (void)hipGetLastError(); c->sw.batch_objects = false; c->err.clear(); break; }
    if (pool && (rc = mf_preallocate_models(c, pool)) != MF_OK) return fail_ctx(rc);
    // the device sections, each checked against its digest
    std::vector<SessSection> secs;
    if ((rc = session_device_sections(c, secs, false, true)) != MF_OK) return fail_ctx(rc);
    if (secs.size() > s.words_cap) return fail(session_refuse("too many sections"));
    LOAD_HIP((hipMemsetAsync(s.d_words, 0, secs.size() * sizeof(unsigned long long), st)));
    std::vector<const SessionEntry*> entries(secs.size(), nullptr);
    const int slot0_sections[3] = {11, 12, 13};
    for (size_t i = 0; i < secs.size(); ++i) {
        SessSection& q = secs[i];
        const SessionEntry* e = entries[i] = session_find(table, q.name.c_str(), q.owner);
        if (!e) return fail(session_refuse("section " + q.name + " is missing"));
        if (q.surfels) {
            ModelState& m = *q.surfels;
            if (e->bytes % 48u || e->bytes / 48u > (uint64_t)m.cap) return fail(session_refuse("section surfels: more surfels than the model's capacity"));
            const int n = (int)(e->bytes / 48u);
            if (fseek(f, (long)e->offset, SEEK_SET) != 0) return fail(session_refuse("cannot read section surfels"));
            const int chunks = (n + kSessionChunk - 1) / kSessionChunk;
            for (int k = 0; k < chunks; ++k) {   // the file read of chunk k runs under the copy and the unpack launch of chunk k - 1
                const int first = k * kSessionChunk, cn = std::min(kSessionChunk, n - first);
                if (k >= 2) LOAD_HIP((hipEventSynchronize(s.ev[k & 1])));
                if (fread(s.h_pin[k & 1], 48, (size_t)cn, f) != (size_t)cn) return fail(session_refuse("cannot read section surfels"));
                LOAD_HIP((hipMemcpyAsync(s.d_stage[k & 1], s.h_pin[k & 1], (size_t)cn * 48, hipMemcpyHostToDevice, st)));
                launch_state_digest(s.d_stage[k & 1], (uint64_t)cn * 48u, (uint64_t)first * 12u, s.d_words + i, st);
                launch_session_unpack(s.d_stage[k & 1], cn, m.surf[0], first, st);
                LOAD_HIP((hipEventRecord(s.ev[k & 1], st)));
            }
            LOAD_HIP((hipStreamSynchronize(st)));
            q.n = n;
            continue;
        }
        void* dst = const_cast<void*>(q.dev);
        uint64_t expect = q.bytes;
        if (q.owner < 0 && ((int)i == slot0_sections[0] || (int)i == slot0_sections[1] || (int)i == slot0_sections[2])) {
            // the last staged frame comes back in input slot 0
            dst = (int)i == 11 ? (void*)c->d_in_rgb[0] : (int)i == 12 ? (void*)c->d_in_depth[0] : (void*)c->d_in_mask[0];
            expect = (int)i == 11 ? P * 3 : (int)i == 12 ? P * sizeof(float) : P;
        }
        if (q.owner >= 0 && q.name == "pose_log") {
            ModelState& m = *c->models[q.owner];
            expect = used_log_entries(c, m) * 8 * sizeof(float);
            if (e->bytes != expect) return fail(session_refuse("section pose_log disagrees with the model's time stamps"));
        }
        if (e->bytes == 0 && expect != 0 && !(q.owner < 0 && (int)i >= 11)) return fail(session_refuse("section " + q.name + " is empty"));
        if ((rc = session_load_block(c, f, *e, dst, expect, s.d_words + i)) != MF_OK) return rc == MF_EINVAL ? fail(rc) : fail_ctx(rc);
    }
    std::vector<unsigned long long> words(secs.size());
    LOAD_HIP((hipMemcpyAsync(words.data(), s.d_words, words.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st)));
    if (hipStreamSynchronize(st) != hipSuccess) { c->err = "mf_session_load: the uploads failed"; return fail_ctx(MF_EHIP); }
    for (size_t i = 0; i < secs.size(); ++i)
        if ((uint64_t)words[i] != entries[i]->digest)
            return fail(session_refuse("section " + secs[i].name + (secs[i].owner >= 0 ? " of model " + std::to_string(secs[i].owner) : std::string()) +
                                       ": the digest does not match its bytes"));
    // the buffers' shape: dense in download order; a fresh table where the saved buffer had one
    for (SessSection& q : secs) {
        if (!q.surfels) continue;
        ModelState& m = *q.surfels;
        hipLaunchKernelGGL(k_session_dense_count, dim3(1), dim3(64), 0, st, m.d_frame, q.n);
        *m.h_count = q.n;
        if (had_table[q.owner]) { launch_run_table(m.surf[0], m.d_frame, st); m.fresh_table(0, (long)q.n); }
        else m.became_dense(0);
    }
    if (c->frame_no > 0) {
        // the Model-level calls read the staged frame through these.  A frame that lay in the caller's memory is not in the file: they then point at
        // zeros in TWO input slots, which staged_slot() does not take for a staged frame -- the next save leaves the frame out again
        c->cur_rgb = c->d_in_rgb[0]; c->cur_depth = staged ? c->d_in_depth[0] : c->d_in_depth[1];
        c->in_slot = 1;
    }
    c->vis_tag.model = nullptr;
    if ((rc = check_launch(c)) != MF_OK) return fail_ctx(rc);
    if (hipStreamSynchronize(st) != hipSuccess) { c->err = "mf_session_load: restoring the buffers failed"; return fail_ctx(MF_EHIP); }
    fclose(f);
    *out = c;
    return MF_OK;
}
#undef LOAD_HIP
