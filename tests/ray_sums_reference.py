"""The reference of the per-ray sums ("Off-axis projection").  It walks nothing of its
own: ray_reference.Hierarchy.rays lists the segments of the field and of the weight, the two lists
must agree in everything but the values, and the four sums are formed from the segments in Python
floats (IEEE binary64, nothing fused), in order.  So it is no twin of the kernel's accumulation: it
rests on a reference that is itself held to geometry (test_rays.py)."""
import math

import numpy as np

GEOMETRY = ("offsets", "status", "t_enter", "t_leave", "t0", "t1", "level")


def same_geometry(a, b):
    return all(a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes()
               for key in GEOMETRY)


def sums_of(start, end, field, weight=None):
    """field, weight (or None): what Hierarchy.rays returned for start -> end.  Returns a dict of
    arrays per ray: count uint32, status uint8, t_enter, t_leave, integral, weight (None without
    one), counted, covered."""
    start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3)
    end = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 3)
    n = start.shape[0]
    assert field["offsets"].size == n + 1
    if weight is not None:
        assert same_geometry(field, weight), "the field and the weight were walked through other cells"
    offsets = field["offsets"]
    out = {"count": np.diff(offsets).astype(np.uint32), "status": field["status"].copy(),
           "t_enter": field["t_enter"].copy(), "t_leave": field["t_leave"].copy(),
           "integral": np.zeros(n), "weight": None if weight is None else np.zeros(n),
           "counted": np.zeros(n), "covered": np.zeros(n)}
    for s in range(n):
        d = [float(end[s, k]) - float(start[s, k]) for k in range(3)]
        square = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        length = math.sqrt(square) if math.isfinite(square) else math.nan
        integral = weight_sum = counted = covered = 0.0
        for i in range(int(offsets[s]), int(offsets[s + 1])):
            if int(field["level"][i]) < 0:
                continue
            w = (float(field["t1"][i]) - float(field["t0"][i])) * length
            v = float(field["value"][i])
            covered = covered + w
            if weight is None:
                if math.isfinite(v):
                    integral = integral + v * w
                    counted = counted + w
            else:
                q = float(weight["value"][i])
                if math.isfinite(v) and math.isfinite(q):
                    integral = integral + (v * q) * w
                    weight_sum = weight_sum + q * w
                    counted = counted + w
        out["integral"][s], out["counted"][s], out["covered"][s] = integral, counted, covered
        if weight is not None:
            out["weight"][s] = weight_sum
    if weight is None:
        # the two sums the walk's own reference forms as well
        assert out["integral"].tobytes() == field["integral"].tobytes()
        assert out["covered"].tobytes() == field["covered"].tobytes()
    return out


def ray_sums(start, end, field_hierarchy, weight_hierarchy=None, max_trips=None):
    """field_hierarchy, weight_hierarchy (or None): ray_reference.Hierarchy of the two fields over
    the same levels."""
    if max_trips is None:
        max_trips = field_hierarchy.default_max_trips()
    field = field_hierarchy.rays(start, end, max_trips)
    weight = None if weight_hierarchy is None else weight_hierarchy.rays(start, end, max_trips)
    return sums_of(start, end, field, weight)
