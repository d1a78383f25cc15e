"""Every reachable build word of the fixed-anchor solve on the MI355X, against the parent's recording: UR10 + table, two
goals, the seven states a fixed-anchor template can be brought into -- plain, links measured only, link hinges, self
hinges, link + self hinges, half-spaces, link hinges + half-spaces.  Per state, gik_template_get_info's whole answer and
the bits of one solve equal tests/golden/anchored_build_words_parent.json (tools/anchored_build_words.py wrote it on the
parent commit).  Nine slots, one wavefront per problem: the smallest shape at which a wrong table row can show -- a row
mix-up changes lds_bytes or anchored at once.  n_cu and waves_per_cu are the MI355X's, compared as recorded."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_graph

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "anchored_build_words_parent.json")
RHO = 0.03
FLOOR = (0.0, 0.0, 1.0, -0.1)
_CAPSULES = dict(link_radius=RHO)
# state -> (what AnchoredProblem is built with, the `anchored` word gik_template_get_info reports)
STATES = {
    "plain": (dict(links=[]), 1),
    "links_measured": (dict(_CAPSULES), 1),
    "link_hinges": (dict(_CAPSULES, link_hinges=True), 3),
    "self_hinges": (dict(_CAPSULES, self_pairs="auto", self_hinges=True), 5),
    "link_self_hinges": (dict(_CAPSULES, self_pairs="auto", link_hinges=True, self_hinges=True), 7),
    "halfspaces": (dict(_CAPSULES, halfspaces=[list(FLOOR)]), 9),
    "link_hinges_halfspaces": (dict(_CAPSULES, link_hinges=True, halfspaces=[list(FLOOR)]), 11),
}


@functools.lru_cache(maxsize=None)
def goals():
    """(robot, graph, q_init [2, 6], goal poses [2, 4, 4]): two configurations of RandomState(9), each asked for the
    pose 0.05 rad further on every joint."""
    robot, graph = make_graph("ur10_table")
    q = np.random.RandomState(9).uniform(-np.pi, np.pi, (2, robot.n))
    return robot, graph, q, robot.fk_batch(q + 0.05)


def run(state):
    """{"info": the template's whole info dict, "x": the solve's points as int64 bit patterns, "shape", "iterations"}"""
    from graphik_amd.solvers import riemannian_solver as rs
    robot, graph, q, T = goals()
    ap = rs.AnchoredProblem(graph, **STATES[state][0])
    res = ap.solve(T, q_init=q)
    x = np.ascontiguousarray(res["x"].detach().cpu().numpy())
    assert x.dtype == np.float64
    return {"info": {k: int(v) for k, v in ap.template.info.items()}, "x": x.view(np.int64).ravel().tolist(),
            "shape": list(x.shape), "iterations": res["iterations"].detach().cpu().numpy().tolist()}


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_table_covers_the_reported_words():
    assert sorted(STATES) == sorted(fixture()["states"])
    assert sorted({w for _, w in STATES.values()}) == [1, 3, 5, 7, 9, 11]


@pytest.mark.parametrize("state", list(STATES))
def test_info_and_solve_equal_the_parent(state):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    want, got = fixture()["states"][state], run(state)
    assert got["info"]["anchored"] == STATES[state][1] and got["info"]["max_terms_per_node"] == 9
    assert got["info"] == want["info"]
    assert got["shape"] == want["shape"] and got["shape"][0] == 2
    assert got["x"] == want["x"]
    assert got["iterations"] == want["iterations"]
