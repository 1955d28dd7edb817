"""The snapshot container of sva_stream_save / sva_stream_load without a GPU (csrc/snapshot/snapshot_format.h through
sva_test_snapshot_header), SlotBook::adopt through sva_test_slot_book, and the parser alone under a host sanitizer.

What is pinned:
  * a header round trip: every field comes back, sva_stream_blob_info agrees, two builds of the same input are byte-identical;
  * every refusal code, and the index of the first differing signature value;
  * every truncation length 0 .. size - 1 of a small blob is refused as truncated, and a blob with a trailing byte is refused too;
  * every single-byte corruption is refused (magic, version, header checksum, payload checksum);
  * SlotBook::adopt against a Python model of the mirrors: over a decoding, a retired and a delay-filling restarted slot;
  * the parser compiled alone with -fsanitize=address,undefined reads nothing past nbytes on the same truncations and corruptions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = [160, 3, 3, 9, 3, 128, 256, 384, 512, 8, 8, 512, 1536, 13, 1, 2, 128, 64, 768, 32, 256]
LAYOUT = [1, 8192, 1, 6, 640, 0, 0, 256, 2, 6, 64, 3, 4096, 32, 262144, 0, 2, 2, 1, 1, 0, -1]
FIELDS = (17, 283, 19, 0, 1)            # frames, last_pos, ncontent, ar_dtype, chunk_frames
NCB, REF_LEN = 8, 11


def _prompt():
    cc = np.arange(REF_LEN, dtype=np.int64) * 37 + 5
    ac = (np.arange(NCB * REF_LEN, dtype=np.int64).reshape(NCB, REF_LEN) * 13) % 1000
    return cc, ac


def _payload(n=48, seed=3):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def blob():
    from streamvoiceanon_amd import engine as E

    cc, ac = _prompt()
    return E.test_snapshot_build(CFG, LAYOUT, FIELDS, cc, ac, _payload())


def test_header_round_trip(blob):
    from streamvoiceanon_amd import engine as E

    cc, ac = _prompt()
    assert blob[:8] == b"SVASNAP1" and len(blob) % 16 == 0
    assert blob == E.test_snapshot_build(CFG, LAYOUT, FIELDS, cc, ac, _payload())          # deterministic: no timestamps, no stray bytes
    rc, field, info = E.test_snapshot_check(blob, CFG, LAYOUT, payload_bytes=48)
    assert (rc, field) == (0, -1)
    assert info == dict(version=1, frames=17, last_pos=283, ncontent=19, ref_len=REF_LEN, ar_dtype=0, chunk_frames=1, payload_bytes=48, ncb=NCB,
                        header_bytes=len(blob) - 48)
    assert blob[info["header_bytes"]:] == _payload()
    # the fixed part and the lists sit where the format says (little-endian)
    assert int.from_bytes(blob[8:12], "little") == 1 and int.from_bytes(blob[16:24], "little") == len(blob)
    assert int.from_bytes(blob[24:32], "little") == 48 and int.from_bytes(blob[68:72], "little") == 283
    off = 104 + 8 * (len(CFG) + len(LAYOUT))
    np.testing.assert_array_equal(np.frombuffer(blob[off:off + 8 * REF_LEN], "<i8"), cc)
    np.testing.assert_array_equal(np.frombuffer(blob[off + 8 * REF_LEN:off + 8 * REF_LEN + 4 * NCB * REF_LEN], "<i4").reshape(NCB, REF_LEN), ac)
    pub = E.stream_blob_info(blob)
    assert pub == {k: info[k] for k in E.SNAPSHOT_INFO}
    # an empty payload and an empty prompt are still a well-formed container
    e = E.test_snapshot_build(CFG, LAYOUT, FIELDS, [], np.zeros((NCB, 0), np.int64), b"")
    assert E.test_snapshot_check(e, CFG, LAYOUT, payload_bytes=0)[0] == 0


def test_every_refusal_code_and_first_differing_field(blob):
    from streamvoiceanon_amd import engine as E

    R = {v: k for k, v in E.SNAPSHOT_REFUSALS.items()}

    def flipped(i, bit=0x01):
        b = bytearray(blob)
        b[i] ^= bit
        return bytes(b)

    hb = len(blob) - 48
    assert E.test_snapshot_check(flipped(0), CFG, LAYOUT)[0] == R["bad_magic"]
    assert E.test_snapshot_check(flipped(8), CFG, LAYOUT)[0] == R["bad_version"]
    assert E.test_snapshot_check(flipped(12), CFG, LAYOUT)[0] == R["bad_header"]           # header length
    assert E.test_snapshot_check(flipped(48), CFG, LAYOUT)[0] == R["bad_header"]           # a count
    assert E.test_snapshot_check(flipped(68), CFG, LAYOUT)[0] == R["bad_header"]           # a scalar field: header checksum
    assert E.test_snapshot_check(flipped(hb - 1), CFG, LAYOUT)[0] in (R["bad_header"],)    # header padding is covered too
    assert E.test_snapshot_check(flipped(hb), CFG, LAYOUT)[0] == R["bad_checksum"]
    assert E.test_snapshot_check(flipped(len(blob) - 1, 0x80), CFG, LAYOUT)[0] == R["bad_checksum"]
    assert E.test_snapshot_check(blob + b"\0", CFG, LAYOUT)[0] == R["bad_header"]
    assert E.test_snapshot_check(blob[:-1], CFG, LAYOUT)[0] == R["truncated"]
    for i in (0, 7, len(CFG) - 1):
        other = list(CFG)
        other[i] += 1
        assert E.test_snapshot_check(blob, other, LAYOUT)[:2] == (R["config_mismatch"], i)
    assert E.test_snapshot_check(blob, CFG[:-2], LAYOUT)[:2] == (R["config_mismatch"], len(CFG) - 2)       # only the lengths differ
    assert E.test_snapshot_check(blob, CFG + [4], LAYOUT)[:2] == (R["config_mismatch"], len(CFG))
    for i in (0, 5, len(LAYOUT) - 1):
        other = list(LAYOUT)
        other[i] -= 1
        assert E.test_snapshot_check(blob, CFG, other)[:2] == (R["layout_mismatch"], i)
    other = list(LAYOUT)
    other[3] += 1
    assert E.test_snapshot_check(blob, CFG[:3] + [0] + CFG[4:], other)[:2] == (R["config_mismatch"], 3)     # the configuration is compared first
    assert E.test_snapshot_check(blob, CFG, LAYOUT, payload_bytes=64)[:2] == (R["size_mismatch"], -1)
    with pytest.raises(ValueError, match="checksum"):
        E.stream_blob_info(flipped(hb))
    with pytest.raises(ValueError, match="truncated"):
        E.stream_blob_info(blob[:50])
    with pytest.raises(ValueError):
        E.stream_blob_info(b"")


def test_every_truncation_and_every_corrupted_byte_is_refused(blob):
    from streamvoiceanon_amd import engine as E

    for n in range(len(blob)):
        rc = E.test_snapshot_check(blob[:n], CFG, LAYOUT)[0]
        assert rc == -10, f"a blob truncated to {n} of {len(blob)} bytes: {E.SNAPSHOT_REFUSALS.get(rc, rc)}"
    for i in range(len(blob)):
        for bit in (0x01, 0x80):
            b = bytearray(blob)
            b[i] ^= bit
            rc = E.test_snapshot_check(bytes(b), CFG, LAYOUT)[0]
            assert rc in (-11, -12, -13, -14), f"byte {i} ^ {bit:#x} of {len(blob)}: {E.SNAPSHOT_REFUSALS.get(rc, rc)}"


# ---- SlotBook::adopt against a model of the mirrors ----------------------------------------------------------------------------
def test_slot_book_adopt_against_python_model():
    from streamvoiceanon_amd import engine as E

    B, chunk, delay, msf, bf, window, nspk = 3, 1, 2, 60, 8, 64, 33
    R0, Ra = 20, 12                             # prompts of the batch, stored prompt of the adopted streams
    ops = [(1, s, R0) for s in range(B)] + [(0, 0, 0), (2, 0, 0), (2, 0, 0), (2, 0, 0)]
    base = len(ops)
    pos, frames = nspk + 2 * Ra - 1 + 2 * delay - 1 + 2 * 5, 5
    ops += [(4, 1, 0), (3, 2, R0), (2, 0, 0),               # slot 1 retired, slot 2 restarted (delay filling), one step
            (6, pos, frames), (7, 0, Ra),                   # over a decoding slot
            (6, pos + 2, frames + 1), (7, 1, Ra),           # over a retired slot
            (6, pos + 4, frames + 2), (7, 2, Ra)]           # over a restarted slot whose delay is filling
    n_adopted = len(ops)
    ops += [(2, 0, 0)] * 40
    t = E.test_slot_book((B, chunk, delay, msf, bf, window, nspk), ops)
    row = t[n_adopted - 1]
    for s, (p, f) in enumerate([(pos, frames), (pos + 2, frames + 1), (pos + 4, frames + 2)]):
        assert tuple(row[4 * s:4 * s + 4]) == (2, p, f, f + delay), f"slot {s} right after its adopt"
    assert row[4 * B] == 1 and t[base - 1][4 * B] == 1            # the batch's lock-step state is not touched
    # model: every adopted slot is an ordinary decoding stream with a stored prompt of Ra frames
    m = [dict(pos=pos + 2 * s, nf=frames + s, nc=frames + s + delay) for s in range(B)]
    redone = 0
    for k in range(n_adopted, len(ops)):
        redo = []
        for s in range(B):
            m[s]["pos"] += 2 * chunk; m[s]["nf"] += chunk; m[s]["nc"] += chunk
            if m[s]["pos"] // 2 >= msf:
                redo.append(s)
                m[s]["pos"] = nspk + 2 * (Ra + min(bf, m[s]["nf"])) - 1 + 2 * delay - 1
        row = t[k]
        for s in range(B):
            assert tuple(row[4 * s:4 * s + 4]) == (2, m[s]["pos"], m[s]["nf"], m[s]["nc"]), f"step {k - n_adopted}, slot {s}"
        assert row[4 * B + 2] == len(redo) and list(row[4 * B + 3:4 * B + 3 + len(redo)]) == redo
        assert row[5 * B + 3] == 0 and row[7 * B + 4] == 0          # nothing parked is rewound, no pending restart is activated: the adopt cleared both
        redone += len(redo)
    assert redone >= B                                               # the re-prefill rule ran on the adopted prompt length


# ---- the parser alone under a host sanitizer --------------------------------------------------------------------------------------
def test_parser_under_address_and_undefined_sanitizers(blob, tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, data = tmp_path / "snapshot_parser", tmp_path / "blob.bin"
    data.write_bytes(blob)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # Probe first, with an empty main: a compiler whose sanitizer runtimes are not installed is the one reason to skip.  The sanitizer runtimes
    # are linked statically where the compiler can (gcc links them dynamically by default), so the program needs nothing from its environment.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx] + san + static + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        static = []
        if subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
            pytest.skip("the host compiler cannot link an empty program with -fsanitize=address,undefined (no sanitizer runtimes)")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + san + static + [os.path.join(ROOT, "tests", "snapshot_parser_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith(f"OK {len(blob)} truncations {2 * len(blob)} corruptions refused")
