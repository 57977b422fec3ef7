"""CPU: the plan-level route switches (plan.switches): one DCAMD_NO_* variable per route, read when a plan is built."""
import pytest

from diffusion_classifier_amd import plan

NAMES = ("PN", "GN_OUT_FUSION", "SKIP_SPLIT", "SHORT_FOLD", "QSTATS", "UP4", "LN_FOLD", "TBLOCK", "PO_FOLD", "TAIL_FOLD", "GN_WS")


@pytest.fixture
def clean(monkeypatch):
    for n in NAMES:
        monkeypatch.delenv("DCAMD_NO_" + n, raising=False)
    return monkeypatch


def test_one_flag_per_variable_and_all_on_by_default(clean):
    sw = plan.switches()
    assert sw._fields == tuple(n.lower() for n in NAMES) and all(sw)
    with pytest.raises(AttributeError):
        sw.pn = False                      # immutable


@pytest.mark.parametrize("value", ["1", ""], ids=["one", "empty"])
@pytest.mark.parametrize("name", NAMES)
def test_each_variable_alone_flips_exactly_its_flag(clean, name, value):
    clean.setenv("DCAMD_NO_" + name, value)             # set, even to the empty string, turns the route off
    sw = plan.switches()
    off = {f for f in sw._fields if not getattr(sw, f)}
    # the loader-side GroupNorm reads the quad records: without them it is off too
    assert off == ({"qstats", "gn_ws"} if name == "QSTATS" else {name.lower()})


def test_two_builds_see_a_change_of_the_environment_in_between(clean):
    assert plan.switches().tblock and not plan.PlanBuilder("cpu", 1, 1, 1).pn_off
    clean.setenv("DCAMD_NO_TBLOCK", "1")
    clean.setenv("DCAMD_NO_PN", "")
    assert not plan.switches().tblock and plan.PlanBuilder("cpu", 1, 1, 1).pn_off
    clean.delenv("DCAMD_NO_PN")
    assert plan.switches().pn and not plan.PlanBuilder("cpu", 1, 1, 1).pn_off
    assert plan.switches(env={"DCAMD_NO_UP4": "0"}) == plan.switches(env={})._replace(up4=False)
