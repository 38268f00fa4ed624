// Sessions through the C++ facade (include/maskfusion/MaskFusion.h: saveSession / loadSession).  One run processes n frames without stopping;
// a second one is saved behind frame `save`, destroyed, loaded and continued.  After every continued frame the two must agree bit for bit in
// the pose, the surfel count and the downloaded map of every model.  Used by tests/test_gpu_session.py.
//   session_main W H fx fy cx cy n_frames save frames.bin session_file
// frames.bin: per frame rgb[H*W*3] u8, depth[H*W] f32.  Prints "session ok <frames compared>" and returns 0 when they agree.
#include <maskfusion/MaskFusion.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

using namespace maskfusion;

struct Frames {
    int W, H;
    std::vector<std::vector<uint8_t>> rgb;
    std::vector<std::vector<float>> depth;
    FrameDataPointer at(int k) {
        auto f = std::make_shared<FrameData>();
        f->timestamp = k; f->index = k; f->rgb = rgb[(size_t)k].data(); f->depth = depth[(size_t)k].data();
        return f;
    }
};

static bool same(MaskFusion& a, MaskFusion& b, int k) {
    if (a.getTick() != b.getTick() || a.getModels().size() != b.getModels().size()) return false;
    auto ia = a.getModels().begin();
    auto ib = b.getModels().begin();
    for (; ia != a.getModels().end(); ++ia, ++ib) {
        const Matrix4f pa = (*ia)->getPose(), pb = (*ib)->getPose();
        if ((*ia)->getID() != (*ib)->getID() || (*ia)->lastCount() != (*ib)->lastCount() || std::memcmp(pa.data(), pb.data(), 16 * sizeof(float))) {
            std::printf("frame %d: model %u differs\n", k, (*ia)->getID());
            return false;
        }
        auto ma = (*ia)->downloadMap(), mb = (*ib)->downloadMap();
        if (ma.numPoints != mb.numPoints || std::memcmp(ma.data->data(), mb.data->data(), (size_t)ma.numPoints * 12 * sizeof(float))) {
            std::printf("frame %d: the map of model %u differs\n", k, (*ia)->getID());
            return false;
        }
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 11) return 1;
    Frames fr;
    fr.W = std::atoi(argv[1]); fr.H = std::atoi(argv[2]);
    const int n = std::atoi(argv[7]), save = std::atoi(argv[8]);
    std::ifstream in(argv[9], std::ios::binary);
    const std::string path = argv[10];
    for (int k = 0; k < n; ++k) {
        fr.rgb.emplace_back((size_t)fr.W * fr.H * 3);
        fr.depth.emplace_back((size_t)fr.W * fr.H);
        in.read((char*)fr.rgb.back().data(), (std::streamsize)fr.rgb.back().size());
        in.read((char*)fr.depth.back().data(), (std::streamsize)(fr.depth.back().size() * sizeof(float)));
        if (!in) return 2;
    }
    Resolution::setResolution(fr.W, fr.H);
    Intrinsics::setIntrinics((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));
    Device::set(0);
    Device::setSurfelBudget(1 << 18, 1 << 16);
    auto make = [] {
        std::unique_ptr<MaskFusion> mf(new MaskFusion(200, 35000, 5e-05f, 1e-05f, false, false, false, 115, 4, 2, 3, 100, false, 0.3095f, false, false, 3));
        mf->setEnableMultipleModels(false);
        return mf;
    };
    auto a = make(), b = make();
    for (int k = 0; k <= save; ++k) {
        a->processFrame(fr.at(k));
        b->processFrame(fr.at(k));
    }
    b->saveSession(path);
    b.reset();                                   // nothing of the saved object is left
    b = MaskFusion::loadSession(path);
    int compared = 0;
    for (int k = save + 1; k < n; ++k, ++compared) {
        a->processFrame(fr.at(k));
        b->processFrame(fr.at(k));
        if (!same(*a, *b, k)) return 3;
    }
    try {                                        // errors are exceptions, as elsewhere
        MaskFusion::loadSession(path + ".missing");
        return 4;
    } catch (const std::runtime_error& e) {
        if (!std::strstr(e.what(), "cannot open")) return 5;
    }
    std::printf("session ok %d\n", compared);
    return 0;
}
