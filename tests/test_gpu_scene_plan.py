"""The handle decides what the pure function decides: rows of tests/test_scene_plan.py's decision table (those marked `gpu`, the three
sequence rows among them) through real handles of 65 arms -- one full wave and a partial one -- with max_slots 16 and 7 joints, in both I/O
types.  A call of the row that names all its arms is repeated over the 65 (arm b takes the row's arm b modulo the row's batch), a partial
call goes to the arms it names; after each set_fields the handle's slots_in_use, field_path, mixed_orders, uniform_repellers and one_chunk
are the table's.  No launch but what creating an engine does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_scene_plan as table  # noqa: E402

pytestmark = pytest.mark.gpu

B = 65
CASES = [(name, knobs, calls, io, want) for name, knobs, calls, wants, gpu in table.ROWS if gpu for io, want in sorted(wants.items())]


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from vfclik_amd import engine, robots
    assert engine.load_library().vfik_device_count() >= 1, "no HIP device: the gpu tests need an MI355X"
    return engine, robots.lwr()


def test_the_rows_are_a_dozen_with_the_sequences():
    names = {c[0] for c in CASES}
    assert len(names) >= 12 and sum(1 for n in names if n.startswith(("28-29", "30"))) == 2
    assert {c[3] for c in CASES} == {32, 64}
    assert all(k.get("nj", 7) == 7 and k.get("S", 16) == 16 for _, k, *_ in CASES)


@pytest.mark.parametrize("case", CASES, ids=["%s-float%d" % (c[0].split(":")[0].replace(" ", "_"), c[3]) for c in CASES])
def test_the_handle_reports_the_tables_plan(env, monkeypatch, case):
    engine, chain = env
    name, knobs, calls, io, want = case
    for var, key in (("VFIK_UNIFORM_IMAGE", "uni"), ("VFIK_MIXED_ORDERS", "mixed"), ("VFIK_ONE_CHUNK", "one")):
        if key in knobs:
            monkeypatch.setenv(var, str(knobs[key]))   # (read when the handle is created)
    eng = engine.Engine(chain, B, io_dtype=np.float32 if io == 32 else np.float64, max_slots=16)
    try:
        rows_batch = knobs.get("B", 1)
        for (first, arms), line in zip(calls, want):
            if first == 0 and len(arms) == rows_batch:
                arms = [arms[b % rows_batch] for b in range(B)]
            f, counts = table.records(arms)
            eng.set_fields(f, counts, first_arm=first)
            w = dict(t.split("=") for t in line.split())
            got = {"slots_used": eng.slots_in_use, "field_path": eng.field_path, "mixed_orders": int(eng.mixed_orders), "uniform": int(eng.uniform_repellers),
                   "one_chunk": int(eng.one_chunk)}
            assert got == {k: (got[k] if w[k] == "*" else int(w[k])) for k in got}, (name, io, line)
    finally:
        eng.close()
