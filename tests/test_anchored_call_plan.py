"""engine.anchored_call_plan: which C entry, which workspace size query and which clearance export behind the entry one
Template.anchored_ik call runs on, for every combination of its keywords that the layer accepts.  The table is written by
hand from the branches Template.anchored_ik had before the plan existed (its docstring states them); it needs no GPU and
no library.

Columns: start (cold / seeded), clearance (off: clearance=False in "nodes"; else clearance=True in that mode), scenes,
retries, retry_candidates, atlas (its atlas_candidates, or -) -> entry (behind "gik_anchored_ik_batch"), size query, after.
Left out, because the layer refuses them: retry_candidates 4 with retries 0, and retry_candidates 4 with an atlas."""
import pytest

from graphik_amd.engine import anchored_call_plan

SIZES = {"ws": "gik_anchored_ws_doubles", "retry": "gik_anchored_retry_ws_bytes",
         "screened": "gik_anchored_ik_batch_retry_screened_ws_bytes", "atlas": "gik_anchored_ik_batch_atlas_ws_bytes"}
AFTER = {"-": None, "nodes": "gik_anchored_clearance", "links": "gik_anchored_link_clearance"}

TABLE = """
cold   off        no  0 1 -   ''               ws       -
cold   nodes      no  0 1 -   ''               ws       nodes
cold   links      no  0 1 -   ''               ws       links
cold   links+self no  0 1 -   _retry           retry    -
seeded off        no  0 1 -   _seeded          ws       -
seeded nodes      no  0 1 -   _seeded          ws       -
seeded links      no  0 1 -   _seeded          ws       links
seeded links+self no  0 1 -   _retry           retry    -
cold   off        yes 0 1 -   _scenes          ws       -
cold   nodes      yes 0 1 -   _scenes          ws       -
cold   links      yes 0 1 -   _scenes          ws       -
cold   links+self yes 0 1 -   _scenes          ws       -
seeded off        yes 0 1 -   _scenes          ws       -
seeded nodes      yes 0 1 -   _scenes          ws       -
seeded links      yes 0 1 -   _scenes          ws       -
seeded links+self yes 0 1 -   _scenes          ws       -
cold   off        no  2 1 -   _retry           retry    -
cold   nodes      no  2 1 -   _retry           retry    -
cold   links      no  2 1 -   _retry           retry    -
cold   links+self no  2 1 -   _retry           retry    -
seeded off        no  2 1 -   _retry           retry    -
seeded nodes      no  2 1 -   _retry           retry    -
seeded links      no  2 1 -   _retry           retry    -
seeded links+self no  2 1 -   _retry           retry    -
cold   off        yes 2 1 -   _retry_scenes    retry    -
cold   nodes      yes 2 1 -   _retry_scenes    retry    -
cold   links      yes 2 1 -   _retry_scenes    retry    -
cold   links+self yes 2 1 -   _retry_scenes    retry    -
seeded off        yes 2 1 -   _retry_scenes    retry    -
seeded nodes      yes 2 1 -   _retry_scenes    retry    -
seeded links      yes 2 1 -   _retry_scenes    retry    -
seeded links+self yes 2 1 -   _retry_scenes    retry    -
cold   off        no  2 4 -   _retry_screened  screened -
cold   nodes      no  2 4 -   _retry_screened  screened -
cold   links      no  2 4 -   _retry_screened  screened -
cold   links+self no  2 4 -   _retry_screened  screened -
seeded off        no  2 4 -   _retry_screened  screened -
seeded nodes      no  2 4 -   _retry_screened  screened -
seeded links      no  2 4 -   _retry_screened  screened -
seeded links+self no  2 4 -   _retry_screened  screened -
cold   off        yes 2 4 -   _retry_screened  screened -
cold   nodes      yes 2 4 -   _retry_screened  screened -
cold   links      yes 2 4 -   _retry_screened  screened -
cold   links+self yes 2 4 -   _retry_screened  screened -
seeded off        yes 2 4 -   _retry_screened  screened -
seeded nodes      yes 2 4 -   _retry_screened  screened -
seeded links      yes 2 4 -   _retry_screened  screened -
seeded links+self yes 2 4 -   _retry_screened  screened -
cold   off        no  0 1 2   _atlas           atlas    -
cold   nodes      no  0 1 2   _atlas           atlas    -
cold   links      no  0 1 2   _atlas           atlas    -
cold   links+self no  0 1 2   _atlas           atlas    -
seeded off        no  0 1 2   _atlas           atlas    -
seeded nodes      no  0 1 2   _atlas           atlas    -
seeded links      no  0 1 2   _atlas           atlas    -
seeded links+self no  0 1 2   _atlas           atlas    -
cold   off        yes 0 1 2   _atlas           atlas    -
cold   nodes      yes 0 1 2   _atlas           atlas    -
cold   links      yes 0 1 2   _atlas           atlas    -
cold   links+self yes 0 1 2   _atlas           atlas    -
seeded off        yes 0 1 2   _atlas           atlas    -
seeded nodes      yes 0 1 2   _atlas           atlas    -
seeded links      yes 0 1 2   _atlas           atlas    -
seeded links+self yes 0 1 2   _atlas           atlas    -
cold   off        no  2 1 2   _atlas           atlas    -
cold   nodes      no  2 1 2   _atlas           atlas    -
cold   links      no  2 1 2   _atlas           atlas    -
cold   links+self no  2 1 2   _atlas           atlas    -
seeded off        no  2 1 2   _atlas           atlas    -
seeded nodes      no  2 1 2   _atlas           atlas    -
seeded links      no  2 1 2   _atlas           atlas    -
seeded links+self no  2 1 2   _atlas           atlas    -
cold   off        yes 2 1 2   _atlas           atlas    -
cold   nodes      yes 2 1 2   _atlas           atlas    -
cold   links      yes 2 1 2   _atlas           atlas    -
cold   links+self yes 2 1 2   _atlas           atlas    -
seeded off        yes 2 1 2   _atlas           atlas    -
seeded nodes      yes 2 1 2   _atlas           atlas    -
seeded links      yes 2 1 2   _atlas           atlas    -
seeded links+self yes 2 1 2   _atlas           atlas    -
"""
ROWS = [tuple(line.split()) for line in TABLE.strip().splitlines()]


def plan_of(start, clearance, scenes, retries, candidates, atlas):
    return anchored_call_plan(start == "seeded", clearance != "off", "nodes" if clearance == "off" else clearance, scenes == "yes",
                              int(retries), int(candidates), None if atlas == "-" else int(atlas))


def test_the_table_covers_every_accepted_combination_once():
    keys = [row[:6] for row in ROWS]
    assert len(set(keys)) == len(keys) == 2 * 4 * 2 * 5      # (retries, candidates, atlas): 5 accepted of 8
    assert {row[3:6] for row in ROWS} == {("0", "1", "-"), ("2", "1", "-"), ("2", "4", "-"), ("0", "1", "2"), ("2", "1", "2")}
    assert len({row[6] for row in ROWS}) == 7 and {row[7] for row in ROWS} == set(SIZES)      # seven entries, four size queries
    assert {row[8] for row in ROWS} == set(AFTER)


@pytest.mark.parametrize("row", ROWS, ids=[" ".join(row[:6]) for row in ROWS])
def test_plan_is_the_parents_branch(row):
    *key, entry, size, after = row
    plan = plan_of(*key)
    assert plan.entry == "gik_anchored_ik_batch" + entry.strip("'")
    assert plan.ws_query == SIZES[size] and plan.after == AFTER[after]
    assert plan.restart == (size != "ws")
    ints = {"ws": (), "retry": (), "screened": (int(key[4]),), "atlas": (int(key[5]) if key[5] != "-" else None, int(key[3]))}[size]
    assert plan.ws_ints == ints


def test_links_self_without_retries_runs_on_the_restart_entry():
    """attempt 0 of gik_anchored_ik_batch_retry alone, on "retry_ws": the entry merges the self clearance into the links'"""
    for start in ("cold", "seeded"):
        plan = plan_of(start, "links+self", "no", 0, 1, "-")
        assert (plan.entry, plan.ws_query, plan.after, plan.restart) == \
            ("gik_anchored_ik_batch_retry", "gik_anchored_retry_ws_bytes", None, True)
        assert plan.args == ("q_init", "B", "opts", "ws", "answer", "clearance", "attempt")
    assert not anchored_call_plan(False, False, "links+self", False, 0).restart      # (no clearance asked for: the cold entry)


def test_atlas_without_retries_runs_on_the_atlas_entry():
    plan = plan_of("cold", "off", "no", 0, 1, 2)
    assert (plan.entry, plan.ws_query, plan.ws_ints, plan.restart) == \
        ("gik_anchored_ik_batch_atlas", "gik_anchored_ik_batch_atlas_ws_bytes", (2, 0), True)
    assert plan.args == ("q_init", "B", "opts", "candidates", "atlas_keys", "atlas_q", "atlas_count", "scenes", "ws", "answer",
                         "clearance", "attempt")


def test_argument_orders_of_the_entries_without_restarts():
    assert plan_of("cold", "nodes", "no", 0, 1, "-").args == ("B", "ws", "answer")
    assert plan_of("seeded", "nodes", "no", 0, 1, "-").args == ("q_init", "B", "ws", "answer", "clearance")
    assert plan_of("seeded", "links", "no", 0, 1, "-").args == ("q_init", "B", "ws", "answer", "null")
    assert plan_of("cold", "links", "yes", 0, 1, "-").args == ("q_init", "B", "scenes", "ws", "answer", "clearance", "mode")
    assert plan_of("seeded", "nodes", "yes", 2, 1, "-").args == ("q_init", "B", "opts", "scenes", "ws", "answer", "clearance", "attempt")
    assert plan_of("cold", "nodes", "no", 2, 4, "-").args == \
        ("q_init", "B", "opts", "candidates", "scenes", "ws", "answer", "clearance", "attempt")
