// Renders through the C++ facade (MaskFusion::renderView, include/maskfusion/MaskFusion.h) after a short stream, for
// tests/test_gpu_render_facade.py, which compares the bytes with the Python call on the same stream.
//   render_main W H fx fy cx cy n_frames frames.bin out.bin
// frames.bin: per frame rgb[H*W*3] u8, depth[H*W] f32, mask[H*W] u8.  out.bin: the follow view at W x H with the camera's focal length, colour types 2 / 4 and the
// palette below: rgba[H*W*4] u8, depth[H*W] f32, model[H*W] i32.
#include <maskfusion/MaskFusion.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>

using namespace maskfusion;

int main(int argc, char** argv) {
    if (argc < 10) {
        std::puts("link ok");
        return 0;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]);
    const float fx = (float)std::atof(argv[3]), fy = (float)std::atof(argv[4]), cx = (float)std::atof(argv[5]), cy = (float)std::atof(argv[6]);
    const int n = std::atoi(argv[7]);
    std::ifstream in(argv[8], std::ios::binary);
    if (!in) return 2;
    Resolution::setResolution(W, H);
    Intrinsics::setIntrinics(fx, fy, cx, cy);
    Device::set(0);
    Device::setSurfelBudget(1 << 18, 1 << 16);
    MaskFusion mf(200, 35000, 5e-05f, 1e-05f, false, false, false, 115, 1, 0.01f, 3, 100, false, 0.3095f, false, false, 3,
                  Model::MatchingType::Drost, Segmentation::Method::MASK_FUSION, "", false, false, 0);
    mf.setEnableMultipleModels(true);
    mf.setTrackAllModels(true);
    mf.setTrackableClassIds({});
    mf.setMfThreshold(0.3f); mf.setMfWeightDistance(150.f); mf.setMfWeightConvexity(2.8f);
    mf.setMfMorphEdgeIterations(0); mf.setMfMorphMaskIterations(0); mf.setNewModelMinRelativeSize(0.004f);
    std::vector<uint8_t> rgb((size_t)W * H * 3), mask((size_t)W * H);
    std::vector<float> depth((size_t)W * H);
    for (int k = 0; k < n; ++k) {
        in.read((char*)rgb.data(), rgb.size());
        in.read((char*)depth.data(), depth.size() * sizeof(float));
        in.read((char*)mask.data(), mask.size());
        if (!in) return 3;
        auto frame = std::make_shared<FrameData>();
        frame->timestamp = k;
        frame->index = k;
        frame->rgb = rgb.data();
        frame->depth = depth.data();
        frame->mask = mask.data();
        frame->classIDs = {0, 41, 42};
        mf.processFrame(frame);
    }
    mf_render_view_t view = mf.defaultRenderView(W, H);
    view.fx = fx;   // the camera's own focal length
    view.fy = fy;
    view.background_color_type = 2;
    view.object_color_type = 4;
    const std::vector<float> palette = {0.9f, 0.1f, 0.1f, 0.1f, 0.8f, 0.2f, 0.2f, 0.3f, 0.95f, 0.9f, 0.8f, 0.1f, 0.6f, 0.2f, 0.7f};
    std::vector<uint8_t> out;
    std::vector<float> z;
    std::vector<int32_t> model;
    mf.renderView(view, out, &z, &model, palette);
    std::ofstream o(argv[9], std::ios::binary);
    o.write((const char*)out.data(), out.size());
    o.write((const char*)z.data(), z.size() * sizeof(float));
    o.write((const char*)model.data(), model.size() * sizeof(int32_t));
    std::printf("models %zu\n", mf.getModels().size());
    return o ? 0 : 4;
}
