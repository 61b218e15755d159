"""What tests/test_gpu_handle_states.py rests on that needs no device: the operation generator is a function of its seed, the
slabs of the scripted tour are what they are meant to be (valid parses, and the two that must be refused each for its one
reason), and the CPU oracle takes the tour's replay arguments: the model alone (tests/_handle_ops.py) follows the tour up to
the first operation whose outcome only the device has, and on the way takes every transition that part is there for."""
import collections

import pytest

import _handle_ops as H
from _libs import Oracle
from _validity import BYTES_DIFFER, NOT_A_PACKET, violations
from megalania_amd import binding, corpus


def test_generator_is_a_function_of_its_seed():
    a, b = H.gen_sequence(7, 40, 8277), H.gen_sequence(7, 40, 8277)
    assert a == b and len(a) == 40
    assert H.gen_sequence(8, 40, 8277) != a
    kinds = collections.Counter(op[0] for s in range(6) for op in H.gen_sequence(s, 40, 8277))
    assert {"run", "mode", "epoch", "set_slab", "set_slab_bad", "seed_greedy", "set_best", "set_best_bad", "set_best_wrong_cost", "cross", "obs",
            "focus", "weights", "live", "temp", "save"} <= set(kinds), kinds
    single = [op for s in range(3) for op in H.gen_sequence(s, 40, 600, single_only=True)]
    assert not any(op[0] == "mode" for op in single)
    for op in single + a:
        if op[0] == "focus":
            assert (op[1], op[2]) == (0, 0) or 0 <= op[1] < op[2] <= 8277


@pytest.mark.parametrize("props", [(0, 0, 0), (3, 0, 2), (0, 4, 2)], ids=lambda p: "lc%d-lp%d-pb%d" % p)
def test_the_named_slabs_are_what_they_are_meant_to_be(props):
    data = corpus.lorem(1800)
    pool = H.Pool(data, props)
    for name in ("literal", "xz"):
        assert violations(data, pool.get(name), H.DICT) == [], name
        assert pool.cost(name) == Oracle(data, *props, dict_limit=H.DICT).cost_slab(pool.get(name))["total"], name
    assert pool.cost("xz") < pool.cost("literal")
    zeroed = H.zeroed_entry(pool.get("xz"))
    assert [c for _, c in violations(data, zeroed, H.DICT)] == [NOT_A_PACKET]
    with pytest.raises(binding.MglError):
        binding.host_cost_map(data, zeroed, props)
    bad = pool.bad_bytes()
    assert [c for _, c in violations(data, bad, H.DICT)] == [BYTES_DIFFER]
    assert int((bad != pool.get("xz")).sum()) == 1


def test_the_oracle_follows_the_tour_up_to_the_device_only_part():
    data = corpus.lorem(1800)
    ops = H.tour()
    device_counts = collections.Counter(H.MET)
    met = collections.Counter()
    model = H.Model(data, H.TOUR_K, H.TOUR_IPE, H.TOUR_SEED, oracle=Oracle(data, dict_limit=H.DICT), counter=met)
    took = H.dry_run(model, H.Pool(data), ops)
    assert ops[took][0] == "seed_greedy" and model.base_is_best, (took, ops[took])
    missing = [t for t in H.TOUR_CPU_PART if not met[t]]
    assert not missing, missing
    # the step with the forced give-up is one that leaves the best slab (the model calls every bulk step a batch accept)
    forced = ops.index(("force_batch_fail",))
    met2 = collections.Counter()
    model = H.Model(data, H.TOUR_K, H.TOUR_IPE, H.TOUR_SEED, oracle=Oracle(data, dict_limit=H.DICT), counter=met2)
    H.dry_run(model, H.Pool(data), ops[:forced])
    before = met2["bulk step leaves the best slab: batch accept"]
    assert model.base_is_best and before >= 1
    H.dry_run(model, H.Pool(data), ops[forced:forced + 2])
    assert met2["bulk step leaves the best slab: batch accept"] == before + 1
    # the live weights' run behind set_slab does not start on a step that refreshes anyway
    live = next(i for i, op in enumerate(ops) if op[0] == "live")
    behind = next(i for i in range(live, len(ops)) if ops[i][0] == "set_slab") + 1
    assert ops[behind][0] == "run" and sum(op[1] for op in ops[:behind] if op[0] == "run") % ops[live][1] != 0
    assert H.MET == device_counts  # nothing here counts for the device cases
