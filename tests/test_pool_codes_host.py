"""CPU: falnet_conv_t::pool_code is not part of the autotune key -- ops.conv_signature of a descriptor does not change with it, and every key of
the committed cache still parses with tests/_conv_ref.parse_signature (a forced-variant launch makes no cache entry of its own)."""
import json
import os

from fal_net_amd import _lib as L
from fal_net_amd import ops

import _conv_ref as R

CACHE = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "autotune_cache.json")


def _keys():
    with open(CACHE) as f:
        return [k for k in json.load(f) if k.startswith("conv|")]


def test_pool_code_is_the_last_field_and_not_in_the_signature():
    assert L.Conv._fields_[-1][0] == "pool_code"
    key = next(k for k in _keys() if R.parse_signature(k)["pool"] and R.parse_signature(k)["pool_mode"] == 0)
    d = R.fill_desc(L.Conv(), R.parse_signature(key))
    assert not d.pool_code and ops.conv_signature(d) == key
    d.pool_code = 0x1000
    assert ops.conv_signature(d) == key
    d.variant = 23  # (nor is the variant: the key names the launch, the cache entry the choice)
    assert ops.conv_signature(d) == key


def test_every_committed_key_still_parses():
    keys = _keys()
    assert len(keys) > 600
    for key in keys:
        sig = R.parse_signature(key)
        assert ops.conv_signature(R.fill_desc(L.Conv(), sig)) == key, key
        assert "pool_code" not in sig
