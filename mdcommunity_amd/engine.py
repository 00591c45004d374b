"""Host-side helpers around the device engine: weight files and shared contexts."""
import os

import numpy as np

from . import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS_DIR = os.path.join(HERE, "weights")

# Reference checkpoint paths (relative to the variant directory, as the scripts name them)
# -> (variant, the fp32 arrays converted from them by scripts/convert_ckpt.py, cost mode).
KNOWN_CKPTS = {
    ("MultiDismantler_unit_cost", "models/g0.5_TORCH-Model_GMM_30_50/nrange_30_50_iter_100000.ckpt"):
        ("unit_g0.5_iter100000.npz", _lib.MD_COST_UNIT),        # U/testSynthetic.py:19
    ("MultiDismantler_unit_cost", "models/g0-1_10w_TORCH-Model_GMM_30_50/nrange_30_50_iter_24000.ckpt"):
        ("unit_g0-1_iter24000.npz", _lib.MD_COST_UNIT),         # U/testReal.py:78-79,100
    ("MultiDismantler_degree_cost", "models/nrange_30_50_iter_100000.ckpt"):
        ("degree_iter100000.npz", _lib.MD_COST_DEGREE),         # D/testReal.py:53,79
}
VARIANT_DIRS = ("MultiDismantler_unit_cost", "MultiDismantler_degree_cost", "CEMultiDismantler", "HCA-Dismantler")
DEFAULT_UNIT = os.path.join(WEIGHTS_DIR, "unit_g0.5_iter100000.npz")
DEFAULT_UNIT_REAL = os.path.join(WEIGHTS_DIR, "unit_g0-1_iter24000.npz")
DEFAULT_DEGREE = os.path.join(WEIGHTS_DIR, "degree_iter100000.npz")
SHIPPED_COST = {npz: cost for npz, cost in KNOWN_CKPTS.values()}


def check_model_rows(rows, model, path):
    """Refuse a checkpoint of the other model: w_n2l has 2 rows in the base (unit / degree cost)
    network and 3 in the community-enhanced one (CEMultiDismantler)."""
    if model is None:
        return
    if model == _lib.MD_MODEL_BASE and rows == 3:
        raise ValueError(f"{path} is a community-enhanced checkpoint (w_n2l has 3 rows); this agent runs the base "
                         "model: use mdcommunity_amd.agent_community (cli variant 'community')")
    if model == _lib.MD_MODEL_COMMUNITY and rows == 2:
        raise ValueError(f"{path} is a base-model checkpoint (w_n2l has 2 rows); the community agent needs a "
                         "CEMultiDismantler checkpoint (w_n2l with 3 rows)")
    if rows not in (2, 3):
        raise ValueError(f"{path}: w_n2l has {rows} rows (expected 2 or 3)")


def _npz_w_n2l_rows(path):
    with np.load(path, allow_pickle=False) as z:
        return int(z["w_n2l"].shape[0]) if "w_n2l" in z.files else None


def resolve_model(path, cost_mode=None, model=None):
    """Map a reference checkpoint path to a loadable file.

    An existing file is returned as is.  Otherwise the path must name one of the reference's
    own checkpoints by its variant-relative path (``./models/...`` as the scripts write it,
    optionally under its variant directory); the shipped .npz converted from it is returned.
    With ``cost_mode`` given, a shipped checkpoint of the other cost model is refused (the
    unit-cost agent must not silently run degree-cost weights, or the reverse).  Anything
    else raises FileNotFoundError.  With ``model`` given (_lib.MD_MODEL_*), a file of the other
    model (by the rows of its w_n2l) is refused: .npz files here, .ckpt files when load_state
    has read them.
    """
    if model == _lib.MD_MODEL_COMMUNITY and (path is None or not os.path.exists(path)):
        raise FileNotFoundError(f"{path}: no community-enhanced checkpoint is shipped; name an existing "
                                "CEMultiDismantler .ckpt or a converted .npz")
    if path is None:
        return DEFAULT_DEGREE if cost_mode == _lib.MD_COST_DEGREE else DEFAULT_UNIT
    if os.path.exists(path):
        shipped = SHIPPED_COST.get(os.path.basename(path))
        if (shipped is not None and cost_mode is not None and shipped != cost_mode
                and os.path.dirname(os.path.abspath(path)) == WEIGHTS_DIR):
            raise ValueError(f"{path} holds {'degree' if shipped else 'unit'}-cost weights; this agent is "
                             f"{'degree' if cost_mode else 'unit'} cost")
        if model is not None and path.endswith(".npz"):
            rows = _npz_w_n2l_rows(path)
            if rows is not None:
                check_model_rows(rows, model, path)
        return path
    norm = os.path.normpath(path.replace("\\", "/")).replace("\\", "/")
    parts = norm.split("/")
    variant = next((d for d in parts if d in VARIANT_DIRS), None)
    for (var, key), (npz, cost) in KNOWN_CKPTS.items():
        if not (norm == key or norm.endswith("/" + key)):
            continue
        if variant is not None and variant != var:
            continue
        if cost_mode is not None and cost != cost_mode:
            raise ValueError(f"{path} is a {'degree' if cost else 'unit'}-cost checkpoint "
                             f"({var}); this agent is {'degree' if cost_mode else 'unit'} cost")
        return os.path.join(WEIGHTS_DIR, npz)
    raise FileNotFoundError(f"{path}: not a file, and not one of the reference's checkpoints "
                            f"({', '.join(k for _, k in KNOWN_CKPTS)})")


def load_state(path, cost_mode=None, model=None):
    """state_dict arrays of a model file: .npz (ours) or a reference .ckpt loaded with
    torch.load(weights_only=True) (U/MultiDismantler_torch.py:791-797)."""
    path = resolve_model(path, cost_mode, model)
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            sd = {k: z[k] for k in z.files}
    else:
        import torch
        sd = torch.load(path, weights_only=True, map_location="cpu")
        sd = {k: v.detach().cpu().numpy() for k, v in sd.items()}
    if model is not None and "w_n2l" in sd:
        check_model_rows(int(np.asarray(sd["w_n2l"]).shape[0]), model, path)
    return sd


def load_weights(path, cost_mode=None, model=None):
    return _lib.pack_weights(load_state(path, cost_mode, model))


_mcc_engine = None


def initial_lmcc(g):
    """Graph_test.max_rank (U/graph.py:80-84) computed by the device MCC (md_reset)."""
    global _mcc_engine
    if _mcc_engine is None:
        _mcc_engine = _lib.Engine(np.zeros(_lib.MD_WEIGHT_FLOATS, np.float32))
    _mcc_engine.load_graphs([(g.num_nodes, g.edges[0], g.edges[1])])
    return int(_mcc_engine.reset()[0])
