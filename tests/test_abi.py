"""The C-ABI library loads and exports exactly the symbols include/maskfusion_amd.h declares (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "maskfusion_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", src)))


def test_header_matches_binding_table():
    from maskfusion_amd.lib import SYMBOLS
    assert header_symbols() == sorted(SYMBOLS)


def test_library_exports_every_symbol():
    from maskfusion_amd import build as b
    from maskfusion_amd.lib import LIB_PATH
    b.build()
    lib = ctypes.CDLL(LIB_PATH)
    for name in header_symbols():
        assert hasattr(lib, name), name


def test_default_config_and_no_gpu_is_loud():
    import ctypes as C
    from maskfusion_amd.lib import load, Config
    L = load()
    cfg = Config()
    assert L.mf_default_config(C.byref(cfg), 640, 480, 528.0, 528.0, 320.0, 240.0) == 0
    assert (cfg.time_delta, cfg.conf_global, cfg.depth_cutoff, cfg.icp_weight) == (200, 4.0, 3.0, 10.0)
    assert cfg.num_gsurfels == 9437184 and cfg.num_osurfels == 1048576
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        assert L.mf_create(C.byref(cfg), C.byref(h)) == -2  # MF_ENODEV: no CPU fallback
        assert not h.value


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "maskfusion_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "mf_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def build_facade_exe(out_dir, lib=None):
    """g++ -std=c++14 tests/cpp/facade_main.cpp against include/ and the shared library -- what INTEGRATION.md asks a MaskFusion
    maintainer to do.  Returns the executable's path.  lib: another build of the same C ABI (the CPU-executed test build of MF_EMU=1)."""
    import subprocess
    lib = lib or os.path.join(ROOT, "maskfusion_amd", "libmaskfusion_amd.so")
    if not os.path.exists(lib):
        from maskfusion_amd import build
        build.build()
    exe = os.path.join(str(out_dir), "facade_main")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_main.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_facade_compiles_and_links(tmp_path):
    """include/maskfusion/MaskFusion.h (the reference's class / method names, constructor argument list, Resolution / Intrinsics
    singletons, listeners, Model-level calls over the C ABI) builds as plain C++14 with -Wall -Wextra -Werror and links against the
    shared library.  (No GPU here: the program only prints "link ok" without arguments; tests/test_gpu_facade.py runs it.)"""
    import subprocess
    exe = build_facade_exe(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "link ok" in out.stdout, out.stderr


def test_cpp_facade_keeps_the_reference_signatures():
    """The facade's constructor takes the reference's 23 arguments in the reference's order (Core/MaskFusion.h:47-53) and the
    Model operations keep their argument lists (Core/Model/Model.h:126-162): checked on the header text."""
    import re
    h = open(os.path.join(ROOT, "include", "maskfusion", "MaskFusion.h")).read()
    ctor = re.search(r"MaskFusion\(int timeDelta = 200,(.*?)\)\s*:", h, re.S).group(0)
    names = ["timeDelta", "countThresh", "errThresh", "covThresh", "closeLoops", "iclnuim", "reloc", "photoThresh", "initConfidenceGlobal",
             "initConfidenceObject", "depthCut", "icpThresh", "fastOdom", "fernThresh", "so3", "frameToFrameRGB", "modelSpawnOffset",
             "matchingType", "segmentationMethod", "exportDirectory", "exportSegmentationResults", "usePrecomputedMasksOnly", "frameQueueSize"]
    pos = [ctor.index(n) for n in names]
    assert pos == sorted(pos)
    for sig in ("performTracking(bool frameToFrameRGB, bool rgbOnly, float icpWeight, bool pyramid, bool fastOdom, bool so3,",
                "fuse(const int& time, GPUTexture*", "clean(const int& time, std::vector<float>&", "predictIndices(int time, float depthCutoff, int timeDelta)",
                "combinedPredict(float depthCutoff, int time, int maxTime, int timeDelta", "SegmentationResult performSegmentation(FrameDataPointer frame)",
                "addNewModelListener(const ModelListener&", "addInactiveModelListener(const ModelListener&", "setTrackableClassIds(const std::set<int>&",
                "makeNonStatic()", "ModelList& getModels()", "bool processFrame(FrameDataPointer frame, const Matrix4f* inPose = nullptr, const float weightMultiplier = 1.f,"):
        assert sig in h, sig


def test_cpp_facade_host_semantics_without_gpu(tmp_path):
    """Frame queue (MaskFusion.cpp:37,206-209), model list as std::list<std::shared_ptr<Model>> with stable identities, new / inactive
    model listeners (MaskFusion.h:303-306), Resolution / Intrinsics preconditions, refusal of what is not built: the facade's host
    logic against a scripted stand-in for the C ABI (tests/cpp/stub_abi.cpp) -- no GPU, no product library involved."""
    import subprocess
    exe = os.path.join(str(tmp_path), "facade_semantics")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_semantics.cpp"), os.path.join(ROOT, "tests", "cpp", "stub_abi.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade semantics ok" in out.stdout, out.stdout + out.stderr


def test_every_parameter_key_is_documented_in_the_header():
    """every key of mf_set_param / mf_get_param -- a row of the table in mf_params.inl -- appears in include/maskfusion_amd.h (rounds 3-5 added
    switches faster than the header learnt of them), and no key is compared against anywhere else"""
    import re
    csrc = os.path.join(ROOT, "maskfusion_amd", "csrc")
    table = open(os.path.join(csrc, "mf_params.inl")).read()
    header = open(os.path.join(ROOT, "include", "maskfusion_amd.h")).read()
    rows = re.findall(r'^    \{"([A-Za-z0-9_]+)", kIn(?:Cfg|Seg|Sw)|^    \{"([A-Za-z0-9_]+)", kComputed', table, re.M)
    keys = [a or b for a, b in rows]
    assert len(keys) == len(set(keys)), sorted(k for k in keys if keys.count(k) > 1)
    missing = sorted(k for k in keys if f'"{k}"' not in header)
    assert len(keys) >= 80 and not missing, missing
    for name in (n for n in os.listdir(csrc) if n.endswith((".hip", ".inl", ".h"))):
        assert not re.search(r'strcmp\(key, "', open(os.path.join(csrc, name)).read()), name
