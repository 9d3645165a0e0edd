"""The model of kmi_index_compare / kmi_index_combine over tests/index_model.CountModel: plain dict arithmetic. Membership is by
key (a stored 0 is present); `ca + cb` follows model_a's reducer (model_a._add: wrap or saturate). Test-side only."""

OPS = ("union_add", "union_max", "intersect_min", "intersect_add", "intersect_left", "subtract_keys", "subtract_counts")
WORDS = ("n_a", "n_b", "n_shared", "sum_a", "sum_b", "sum_a_shared", "sum_b_shared", "sum_min_shared")


def _ratio(num, den):
    return num / den if den else 0.0


def overlap(model_a, model_b):
    """the dict CountIndex.compare returns: the eight integer words and the four ratios"""
    a, b = model_a.d, model_b.d
    shared = [key for key in a if key in b]
    o = {"n_a": len(a), "n_b": len(b), "n_shared": len(shared), "sum_a": sum(a.values()), "sum_b": sum(b.values()),
         "sum_a_shared": sum(a[key] for key in shared), "sum_b_shared": sum(b[key] for key in shared),
         "sum_min_shared": sum(min(a[key], b[key]) for key in shared)}
    o["jaccard"] = _ratio(o["n_shared"], o["n_a"] + o["n_b"] - o["n_shared"])
    o["containment_a"] = _ratio(o["n_shared"], o["n_a"])
    o["containment_b"] = _ratio(o["n_shared"], o["n_b"])
    o["weighted_jaccard"] = _ratio(o["sum_min_shared"], o["sum_a"] + o["sum_b"] - o["sum_min_shared"])
    return o


def combined(model_a, model_b, op):
    """a copy of model_a after combine(model_b, op); model_b is not touched"""
    assert op in OPS, op
    a, b = model_a.d, model_b.d
    out = model_a.copy()
    if op == "union_add":
        out.d = {key: model_a._add(a.get(key, 0), b.get(key, 0)) for key in list(a) + [key for key in b if key not in a]}
    elif op == "union_max":
        out.d = {key: max(a.get(key, 0), b.get(key, 0)) for key in list(a) + [key for key in b if key not in a]}
    elif op == "intersect_min":
        out.d = {key: min(c, b[key]) for key, c in a.items() if key in b}
    elif op == "intersect_add":
        out.d = {key: model_a._add(c, b[key]) for key, c in a.items() if key in b}
    elif op == "intersect_left":
        out.d = {key: c for key, c in a.items() if key in b}
    elif op == "subtract_keys":
        out.d = {key: c for key, c in a.items() if key not in b}
    else:   # subtract_counts: an absent key counts 0, so a stored 0 of a leaves too
        out.d = {key: c - b.get(key, 0) for key, c in a.items() if c > b.get(key, 0)}
    return out
