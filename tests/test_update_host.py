"""de_program_update on the host side (no GPU): the header's declaration, Population.update's argument checks and the id mapping of a
sharded population (dist.shard_update)."""
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api, dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_de_program_update():
    h = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    m = re.search(r"int\s+de_program_update\s*\(([^)]*)\)\s*;", h)
    assert m, "de_program_update is not declared"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["de_program_t *prog", "const int64_t *tree_ids", "int64_t n_update", "const de_tape_node_t *nodes",
                      "const int64_t *node_offsets", "const de_tape_node_t *cse_nodes", "const int64_t *cse_offsets",
                      "const void *consts", "const int64_t *const_offsets"]
    assert "#define DE_HIP_ABI_VERSION 3" in h
    assert "de_program_update" in h[:h.index("#define DE_HIP_ABI_VERSION")], "the addition belongs in the 'Additive since' list"
    assert "de_program_update" in api.EXPORTS


def test_update_ids_are_checked_before_the_library_is_called():
    assert api.check_update_ids([], 0, 10).dtype == np.int64
    ids = api.check_update_ids([3, 0, 9], 3, 10)
    assert ids.dtype == np.int64 and ids.tolist() == [3, 0, 9]
    assert api.check_update_ids(np.array([9], dtype=np.uint8), 1, 10).tolist() == [9]
    assert api.check_update_ids(range(10), 10, 10).tolist() == list(range(10))
    for bad, n_new in [([1, 1], 2), ([10], 1), ([-1], 1), ([1, 2], 3), ([1.0], 1), ([[1]], 1)]:
        with pytest.raises(ValueError):
            api.check_update_ids(bad, n_new, 10)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_update_maps_global_ids_to_local_ones(world):
    n = 37
    ids = [0, 5, 36, 17, 8, 9, 30]
    trees = [f"tree{t}" for t in ids]
    seen = []
    for rank in range(world):
        local, got = dist.shard_update(ids, trees, rank, world)
        owned = dist.shard_indices(n, rank, world)
        assert len(local) == len(got)
        for li, tr in zip(local, got):
            g = owned[li]  # the shard's local index li is global tree owned[li]
            assert tr == f"tree{g}" and g % world == rank
            seen.append(g)
    assert sorted(seen) == sorted(ids)
    with pytest.raises(ValueError):
        dist.shard_update([1, 2], ["a"], 0, world)
    with pytest.raises(ValueError):
        dist.shard_update([1], ["a"], world, world)
