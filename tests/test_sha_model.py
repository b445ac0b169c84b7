"""tests/sha_model.py against hashlib: the restated compression is the reference for every state
the suite hands to the GPU hash queue, so its own chain, finished with the padding of FIPS 180-4
§5.1.1, must give hashlib's digest at the padding edges."""
import hashlib

import numpy as np
import pytest

from tests.sha_model import IV, _compress, state_after


@pytest.mark.parametrize("length", [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 64 * 40 + 17])
def test_state_after_then_padding_is_hashlib(length):
    msg = np.random.default_rng(length).integers(0, 256, length, dtype=np.uint8).tobytes()
    padded = msg + b"\x80" + b"\0" * ((55 - length) % 64) + (8 * length).to_bytes(8, "big")
    assert len(padded) % 64 == 0
    assert state_after(msg, 0) == IV
    for start in sorted({0, length // 64 // 2, length // 64}):
        h = state_after(msg, start)
        assert h == state_after(padded, start)      # bytes past the blocks asked for are not read
        for o in range(64 * start, len(padded), 64):
            h = _compress(h, padded[o:o + 64])
        assert "".join("%08x" % x for x in h) == hashlib.sha256(msg).hexdigest()
