"""The canonical order of the swarm (include/jaybenne_amd.h: jb_set_cell_order, JB_CELL_ORDER_BY_ID) restated in
numpy, from its rule -- never from the library: slots by (sort key, id, input slot), the sort key that of
``comb_model.cell_keys`` and the id a full unsigned 64-bit word."""
import numpy as np

import comb_model as cm


def canonical_order(mesh, local_gids, sw, n: int):
    """(order, key): ``order[r]`` = the input slot that belongs in slot r; key per input slot."""
    key, _, _, _ = cm.cell_keys(mesh, local_gids, sw, n)
    ids = np.ascontiguousarray(sw["id"][:n]).view(np.uint64)
    return np.lexsort((np.arange(n), ids, key)), key


def canonical_sort(mesh, local_gids, sw, n: int):
    """The first n slots of every array in canonical order."""
    order, _ = canonical_order(mesh, local_gids, sw, n)
    return {k: np.ascontiguousarray(sw[k][:n][order]) for k in cm.SWARM_KEYS}


def is_canonical(mesh, local_gids, sw, n: int) -> bool:
    order, _ = canonical_order(mesh, local_gids, sw, n)
    return bool(np.array_equal(order, np.arange(n)))
