"""CPU-only: the state blob's header (include/f110.h, f110_state_*) as f1tenth_gym_amd.StateBlob parses and validates it, and
its to_bytes / from_bytes round trip.  The blobs here are built by hand in the documented layout — no device involved."""
import numpy as np
import pytest


def _blob(k=3, A=2, B=1080, cols=1 | 4, flags=0, body=512, **over):
    from f1tenth_gym_amd.core import STATE_HEADER
    h = np.zeros(1, dtype=STATE_HEADER)
    h["magic"], h["version"], h["k"], h["A"], h["B"], h["flags"], h["cols"] = b"F110SNAP", 1, k, A, B, flags, cols
    h["noise_mode"], h["noise_rows"], h["n_maps"], h["ego_idx"], h["max_step"] = 2, 16384, 0, -1, 151
    h["noise_id"] = [1, 2, 3, 4]
    h["std_dev"] = 0.01
    for key, v in over.items():
        h[key] = v
    raw = np.concatenate([h.view(np.uint8), np.arange(body, dtype=np.uint8)])
    if "total_bytes" not in over:
        raw[:256].view(STATE_HEADER)["total_bytes"] = raw.nbytes
    return raw


def test_header_layout_is_256_bytes_with_the_documented_offsets():
    from f1tenth_gym_amd.core import STATE_HEADER
    assert STATE_HEADER.itemsize == 256
    offs = {n: STATE_HEADER.fields[n][1] for n in STATE_HEADER.names}
    assert offs["version"] == 8 and offs["k"] == 12 and offs["cols"] == 28 and offs["noise_mode"] == 32
    assert offs["max_step"] == 48 and offs["noise_id"] == 56 and offs["std_dev"] == 88 and offs["total_bytes"] == 96


def test_header_is_parsed():
    from f1tenth_gym_amd import StateBlob
    b = StateBlob(_blob(k=5, cols=1 | 2 | 4 | 16, flags=1))
    h = b.header
    assert (h["num_envs"], h["num_agents"], h["num_beams"]) == (5, 2, 1080)
    assert h["scans"] and h["columns"] == ("agent", "scans", "rng", "episode")
    assert h["noise_mode"] == "shared_rng" and h["noise_id"] == (1, 2, 3, 4) and h["std_dev"] == 0.01
    assert h["max_step"] == 151 and h["ego_idx"] == -1 and h["total_bytes"] == b.nbytes == 256 + 512
    assert b.num_envs == 5 and "5 envs x 2 agents" in repr(b)


def test_to_bytes_from_bytes_round_trip():
    from f1tenth_gym_amd import StateBlob
    raw = _blob()
    b = StateBlob(raw)
    data = b.to_bytes()
    assert isinstance(data, bytes) and data == raw.tobytes()
    c = StateBlob.from_bytes(data)
    assert np.array_equal(c.data, b.data) and c.header == b.header
    assert StateBlob(bytearray(data)).header == b.header   # any buffer of bytes
    c.data[300] ^= 1                                      # from_bytes owns its copy
    assert b.data[300] == raw[300]


@pytest.mark.parametrize("damage,msg", [
    (lambda r: r.__setitem__(0, ord("X")), "bad magic"),
    (lambda r: r[:256].view("<u4").__setitem__(2, 7), "format version 7"),
    (lambda r: None, "at least 256 bytes"),
    (lambda r: r[:256].view("<u8").__setitem__(12, 5), "its header says 5"),
])
def test_corrupted_blobs_are_refused(damage, msg):
    from f1tenth_gym_amd import StateBlob
    raw = _blob()
    if msg == "at least 256 bytes":
        raw = raw[:100]
    damage(raw)
    with pytest.raises(ValueError, match=msg):
        StateBlob(raw)
    with pytest.raises(ValueError):
        StateBlob.from_bytes(raw.tobytes())


def test_truncated_blob_is_refused():
    from f1tenth_gym_amd import StateBlob
    raw = _blob()
    with pytest.raises(ValueError, match="state blob of 700 bytes"):
        StateBlob(raw[:700])
    with pytest.raises(ValueError, match="1-D uint8"):
        StateBlob(raw.view(np.uint16))
