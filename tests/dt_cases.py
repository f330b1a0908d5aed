"""Cases at a network dt other than 1: the simulated time of a run of T steps, the id suffix of such a case, and what a fixture
generator asserts on the reference's own record before it keeps one.  Network.run takes `int(time / dt)` steps; where the product
T * dt does not divide back to T in double precision (T = 31 at dt 0.3, T = 43 at dt 0.1, ...), half a step of slack is added."""
import os

import numpy as np


def run_time(T, dt):
    """`time` such that int(time / dt) == T: T itself at dt = 1 (the existing fixtures' call), else T * dt, plus half a step where
    the division would fall one short."""
    if dt == 1.0:
        return T
    time = T * dt
    if int(time / dt) != T:
        time = (T + 0.5) * dt
    assert int(time / dt) == T, (T, dt, time)
    return time


def tag(dt):
    """The id suffix of a case at dt: 0.5 -> "dt05", 2.0 -> "dt2", 0.1 -> "dt01", 0.3 -> "dt03"."""
    s = ("%g" % dt).replace(".", "")
    return "dt" + s


def again(raster):
    """How many neurons of a [T, B, n] raster fire three or more times in one sample: a refractory period ended and the neuron fired
    again, twice."""
    return int((raster.reshape(raster.shape[0], raster.shape[1], -1).sum(axis=0) >= 3).any(axis=0).sum())


def save_fixture(path, out, name, rasters, sibling_path, refractory, also=(), band=(0.005, 0.7)):
    """The one place a generator keeps the fixture of a dt != 1 case: `out` is written to `path` only if the reference's own record meets
    every condition.  rasters: one [T, B, n] array per input of the case.
      * the spike rate over all inputs lies inside `band`;
      * refractory (the layer has a refractory period): in EVERY input at least 10 neurons fire three or more times in one sample;
      * nothing stored, and none of the records `also` that are stored as a hash only, is NaN or infinite;
      * the file is no larger than its dt = 1 sibling's (sibling_path; None where the case has none).
    A case that misses one changes its input or its T, never the condition.  Returns (rate, [neurons with >= 3 spikes per input])."""
    rasters = [np.asarray(r) for r in rasters]
    rate = sum(int(r.sum()) for r in rasters) / sum(r.size for r in rasters)
    assert band[0] < rate < band[1], f"case {name}: spike rate {rate}"
    counts = [again(r) for r in rasters]
    assert not refractory or min(counts) >= 10, f"case {name}: neurons with three or more spikes, per input: {counts}"
    bad = [k for k, a in out.items() if isinstance(a, np.ndarray) and a.dtype.kind == "f" and not np.isfinite(a).all()]
    bad += [f"also[{i}]" for i, a in enumerate(also) if not np.isfinite(np.asarray(a)).all()]
    assert not bad, f"case {name}: NaN or infinity in {bad}"
    tmp = path[:-len(".npz")] + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    size, limit = os.path.getsize(tmp), None if sibling_path is None else os.path.getsize(sibling_path)
    if limit is not None and size > limit:
        os.remove(tmp)
        raise AssertionError(f"case {name}: {size} bytes, larger than its dt = 1 sibling ({limit})")
    os.replace(tmp, path)
    print(f"  {name}: rate {rate:.3f}, neurons with >= 3 spikes per input {counts}, {size} bytes")
    return rate, counts
