"""The switch of the fp32 search direction (remo_debug_tune key 41) and the getter that says which storage the last solve used are part
of the product library; what they do on the GPU is tests/test_gpu_direction_fp32.py."""


def test_key_41_is_in_the_product_library():
    from remo3d_amd import _lib
    L = _lib.load()
    assert L.remo_debug_tune(41, 1) == 0
    assert L.remo_debug_tune(41, 0) == 0
    assert L.remo_debug_tune(41, 1) == 0     # (back to the default)


def test_direction_bytes_getter_is_exported():
    from remo3d_amd import _lib
    L = _lib.load()
    assert "remo_debug_direction_bytes" in _lib.DEBUG_EXPORTS
    assert hasattr(L, "remo_debug_direction_bytes")
    assert L.remo_debug_direction_bytes(None) < 0     # no context: an argument error, not a crash
