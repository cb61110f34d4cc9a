"""GAEngine declares its state up front: every attribute it ever holds is assigned in __init__ (None / False where the object is
built on first use, or by setup_device_loop), so no call order decides whether an attribute exists.  On the CPU, under the
launch-script driver's stubs (tests/golden/make_golden_launches.py), with the built library."""
import importlib.util
import inspect
import os
import re

import pytest


@pytest.fixture(scope="module")
def driver(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_launches", os.path.join(golden_dir, "make_golden_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def stubs(driver):
    """(driver, the names of the entry points called so far): the driver's stubs for the length of the test, the library's call
    replaced by a list of names (a download writes into a tensor the engine does not keep, which the recorder refuses)"""
    from coevonet_amd import lib as L
    calls = []
    with driver.stubbed():
        driver.REC.log, driver.REC.es, driver.REC.n_ro = [], False, 0
        L.call = lambda name, *args: calls.append(name)
        yield driver, calls
    driver.REC.log = []


def test_a_fresh_engine_answers_what_needs_no_device_loop(stubs):
    driver, calls = stubs
    eng = driver._ga(6, 2, 2, cohorts=2)
    eng.flush_breeding()                                 # nothing pending: nothing launched
    assert calls == []
    assert eng.download("agent_0", "pop", 0, 1).shape == (1, eng.P["agent_0"])
    assert eng._packed_exchange() is False
    eng.select()
    assert calls == ["coevo_fc_unpack"] + ["coevo_fc_distance"] * 3 + ["coevo_ga_select"]


@pytest.mark.parametrize("method", ["step_sharded", "replay_generation", "replay_generation_pipelined", "enqueue_generation"])
def test_a_device_loop_method_without_setup_raises_one_runtime_error_that_names_the_call(stubs, method):
    driver, calls = stubs
    eng = driver._ga(6, 2, 2, cohorts=2)
    with pytest.raises(RuntimeError, match=r"setup_device_loop\(args, capacity\)"):
        getattr(eng, method)(*(() if method == "enqueue_generation" else (0,)))
    assert calls == [] and driver.REC.log == []          # ... before anything was launched or asked of the rollout
    eng.setup_device_loop(driver.LOOP_ARGS, 16)
    eng.replay_generation(0)                             # (the stub rollout has use_graph False: enqueue_generation)
    assert calls[-1] == "coevo_counter_add"


def test_setup_device_loop_adds_no_attribute_and_neither_does_a_generation_of_any_path(stubs):
    driver, calls = stubs
    eng = driver._ga(6, 2, 2)                            # (one cohort: the cohort chains need real streams)
    declared = set(vars(eng))
    eng.setup_device_loop(driver.LOOP_ARGS, 16)
    for gen in range(2):
        eng.replay_generation(gen)
        eng.step_sharded(gen)
        eng.rollout(gen, with_prev_eval=gen > 0)
        eng.select()
        eng.breed_device(gen, driver.SIG3)
    assert set(vars(eng)) == declared and "coevo_ga_select_adapt" in calls and "coevo_ga_select" in calls


def test_the_engine_reads_its_state_without_lazy_idioms():
    from coevonet_amd import genetic_algorithm, population
    lazy = re.compile(r'getattr\(self, "\w+", |self\.__dict__\.setdefault|hasattr\(self\.ro\b')
    for src in (inspect.getsource(genetic_algorithm), inspect.getsource(population.CoGATail)):
        assert lazy.findall(src) == []
    assert population.CoGATail._hof_tiled is False
