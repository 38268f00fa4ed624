"""The session file format as include/maskfusion_amd.h documents it, without a GPU: a file built here from that description alone is read by
mf_session_info, and malformed variants are refused with MF_EINVAL and a reason."""
import ctypes as C
import struct

import numpy as np
import pytest

MAGIC = b"MFSESSN1"


def digest(data: bytes) -> int:
    """little-endian 32-bit words w_i of the bytes (tail zero-padded): sum (w_i + 1) (2 i + 1) mod 2^64"""
    data += b"\0" * (-len(data) % 4)
    w = np.frombuffer(data, "<u4").astype(np.uint64)
    i = np.arange(len(w), dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((w + np.uint64(1)) * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64))


def build_file(sizes, user=b"frame 17", sections=(), version=1, magic=MAGIC, W=328, H=248, models=3, tick=18, frames=17):
    """header (64 bytes) | section table (64 bytes per section) | payloads at multiples of 256"""
    sections = list(sections) + [("user", -1, user)]
    header = struct.pack("<8sIIIIiiiiQIIq", magic, version, sizes["pose"], sizes["frame"], sizes["run"], W, H, models, tick, len(user), len(sections),
                         sizes["config"], frames)
    assert len(header) == 64
    at = (64 + 64 * len(sections) + 255) // 256 * 256
    table, body = b"", b""
    for name, owner, payload in sections:
        table += struct.pack("<32siIQQQ", name.encode(), owner, 0, at, len(payload), digest(payload))
        body += payload + b"\0" * (-len(payload) % 256)
        at += (len(payload) + 255) // 256 * 256
    pad = (64 + len(table) + 255) // 256 * 256 - 64 - len(table)
    return header + table + b"\0" * pad + body


@pytest.fixture(scope="module")
def lib():
    from maskfusion_amd.lib import load
    return load()


@pytest.fixture(scope="module")
def sizes(lib, tmp_path_factory):
    """what this build was compiled with: its refusal of a header that carries other sizes names them -- 'this build has a / b / c / d'"""
    p = str(tmp_path_factory.mktemp("probe") / "probe.mfs")
    open(p, "wb").write(build_file(dict(pose=1, frame=1, run=1, config=1)))
    from maskfusion_amd.lib import SessionInfo
    assert lib.mf_session_info(p.encode(), C.byref(SessionInfo()), None, 0, None) == -1
    why = lib.mf_last_error(None).decode()
    a, b, c, d = [int(v) for v in why.split("this build has")[1].split("/")]
    return dict(pose=a, frame=b, config=c, run=d)


def info(lib, path, capacity=64):
    from maskfusion_amd.lib import SessionInfo
    out, n, blob = SessionInfo(), C.c_uint64(0), C.create_string_buffer(capacity)
    rc = lib.mf_session_info(str(path).encode(), C.byref(out), blob, capacity, C.byref(n))
    return rc, out, blob.raw[:min(capacity, n.value)], n.value, (lib.mf_last_error(None) or b"").decode()


def test_a_header_built_from_the_documented_format_is_read(lib, sizes, tmp_path):
    user = b"{\"frames\": 17}"
    p = tmp_path / "ok.mfs"
    p.write_bytes(build_file(sizes, user=user, sections=[("surfels", 0, bytes(range(96))), ("context", -1, b"abc")]))
    rc, out, blob, n, why = info(lib, p)
    assert rc == 0, why
    assert (out.version, out.width, out.height, out.n_models, out.tick, out.frames, out.n_sections) == (1, 328, 248, 3, 18, 17, 3)
    assert (out.pose_bytes, out.frame_bytes, out.run, out.config_bytes) == (sizes["pose"], sizes["frame"], sizes["run"], sizes["config"])
    assert blob == user and n == len(user) and out.user_bytes == len(user) and out.file_bytes == p.stat().st_size
    rc, _, blob, n, _ = info(lib, p, capacity=4)          # a smaller buffer receives the head of the blob and still learns its size
    assert rc == 0 and blob == user[:4] and n == len(user)
    from maskfusion_amd import MaskFusion
    d = MaskFusion.sessionInfo(str(p))
    assert d["user"] == user and (d["width"], d["height"], d["n_models"], d["tick"]) == (328, 248, 3, 18)


def test_an_empty_user_blob(lib, sizes, tmp_path):
    p = tmp_path / "empty.mfs"
    p.write_bytes(build_file(sizes, user=b""))
    rc, out, blob, n, why = info(lib, p)
    assert rc == 0 and blob == b"" and n == 0 and out.user_bytes == 0, why


@pytest.mark.parametrize("name,word", [("short_header", "short"), ("short_table", "short"), ("short_payload", "short"), ("magic", "magic"), ("version", "version"),
                                       ("pose_size", "sizeof(PoseDev)"), ("run", "run length"), ("blob_byte", "digest"), ("no_blob", "missing"),
                                       ("missing_file", "cannot open")])
def test_malformed_files_are_refused(lib, sizes, tmp_path, name, word):
    good = build_file(sizes, user=b"0123456789" * 40, sections=[("surfels", 0, bytes(480))])
    table = 64 + 64 * 2
    blob_at = struct.unpack_from("<Q", good, 64 + 64 + 40)[0]
    data = {
        "short_header": good[:40],
        "short_table": good[:table - 8],
        "short_payload": good[:blob_at + 100],
        "magic": b"MFSESSN2" + good[8:],
        "version": build_file(sizes, version=2),
        "pose_size": build_file(dict(sizes, pose=sizes["pose"] + 4)),
        "run": build_file(dict(sizes, run=sizes["run"] * 2)),
        "blob_byte": good[:blob_at + 7] + bytes([good[blob_at + 7] ^ 1]) + good[blob_at + 8:],
        "no_blob": build_file(sizes).replace(b"user" + b"\0" * 28, b"usex" + b"\0" * 28),
        "missing_file": None,
    }[name]
    p = tmp_path / (name + ".mfs")
    if data is not None:
        p.write_bytes(data)
    rc, _, _, _, why = info(lib, p)
    assert rc == -1 and word in why, (name, why)          # MF_EINVAL and a reason
    from maskfusion_amd import MaskFusion
    from maskfusion_amd.lib import MFError
    with pytest.raises(MFError):
        MaskFusion.sessionInfo(str(p))
