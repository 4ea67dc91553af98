"""CPU: rotation schedules in the stored-ciphertext hub, the
parts that need no GPU: header, library and binding agree on the two new
entries and their structs; what they refuse before they look at a group; and
CorpusHub(rotation_schedules=True) against stub servers: a multi-bridge rekey
is accepted, a missing generation's fingerprint is named with the tenant, the
items handed to the group carry each tenant's (ends, slots), and the default
hub still calls the one-old-generation entry.

A group cannot be created on host-only contexts (fhe_group_create stops at
their missing keys, tests/test_group_cpu.py pins that), so the per-tenant
FHE_E_ARG order of the new entries is checked on the device, on engines that
hold no packing or bridge key: tests/test_gpu_hub_gens.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from fheicp import _lib
from test_bridge_gens_cpu import StubEngine, fake_keys, stub_server  # noqa: F401  (stub_server is a fixture)

U = np.uint64
E_ARG = -1
HDR = (Path(__file__).resolve().parents[1] / "include" / "fhe_icp.h").read_text()


def header_fields(name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", HDR, re.S).group(1)
    return re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_header_library_and_binding_agree():
    L = _lib.lib()
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name, nargs in (("fhe_bridge_group_gens_batch", 5), ("fhe_search_seeded_queries_group_gens_batch", 4)):
        decl = re.search(r"\bint " + name + r"\((.*?)\);", HDR, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(bound[name][1]), name
        assert getattr(L, name).argtypes == bound[name][1]
    assert header_fields("fhe_group_rowmap") == [f for f, _ in _lib.FheGroupRowmap._fields_]
    assert header_fields("fhe_group_rowmap") == ["struct_size", "G", "Q", "B", "h_ends", "h_slots"]
    assert C.sizeof(_lib.FheGroupRowmap) == 40
    gens = header_fields("fhe_group_corpus_gens")
    assert gens == [f for f, _ in _lib.FheGroupCorpusGens._fields_] and gens[0] == "struct_size"
    # fhe_group_corpus with the row map in B_old's place; fhe_group_corpus itself keeps its layout
    old = header_fields("fhe_group_corpus")
    assert set(gens) - {"G", "h_ends", "h_slots"} == set(old) - {"B_old", "reserved"}
    assert old == [f for f, _ in _lib.FheGroupCorpus._fields_] and C.sizeof(_lib.FheGroupCorpus) == 104
    assert C.sizeof(_lib.FheGroupCorpusGens) == 112


def test_new_entries_reject_a_null_group():
    L = _lib.lib()
    maps = (_lib.FheGroupRowmap * 1)()
    assert L.fhe_bridge_group_gens_batch(None, None, maps, 1, None) == E_ARG
    assert b"group" in L.fhe_last_error(None)
    assert L.fhe_search_seeded_queries_group_gens_batch(None, None, 1, None) == E_ARG
    assert b"group" in L.fhe_last_error(None)


# ------------------------------------------------- CorpusHub, stub servers --
class StubGroup:
    """Stands for EngineGroup in CorpusHub: records the entry and the items."""

    def __init__(self, servers):
        self.servers, self.calls = servers, []

    def _run(self, entry, items):
        self.calls.append((entry, items))
        return [None if it is None else s.engine._reply(it[0], it[5]) for s, it in zip(self.servers, items)]

    def search_seeded_queries(self, items):
        return self._run("one", items)

    def search_seeded_queries_gens(self, items):
        return self._run("gens", items)

    def close(self):
        pass


def docs_of(rng, n):
    return rng.integers(0, 2 ** 64, (n, 16), dtype=U), rng.integers(0, 2 ** 64, n, dtype=U)


def ids_of(n):
    from fheicp.stored import key_fingerprint
    return [key_fingerprint(fake_keys(g)["ksk"]) for g in range(n)]


def make_hub(stub_server, schedules, names):  # noqa: F811
    from fheicp.stored import CorpusHub
    hub = CorpusHub(0, rotation_schedules=schedules) if schedules is not None else CorpusHub()
    for name in names:
        hub.add_tenant(name, None, None, 0, None, server=stub_server(fake_keys(0)))
    hub._group = StubGroup(list(hub.tenants.values()))
    return hub


def test_schedules_hub_accepts_multi_bridge_rekeys_and_names_the_tenant(stub_server):  # noqa: F811
    id0, id1, id2, id3 = ids_of(4)
    hub = make_hub(stub_server, True, ("alice", "bob"))
    rng = np.random.default_rng(2)
    hub.load("alice", *docs_of(rng, 12))
    hub.rekey("alice", fake_keys(1, bridge_from=id0))                # the single form goes to the server as before
    hub.append("alice", *docs_of(rng, 5))
    s = hub.tenants["alice"]
    n_imp = len(s.engine.imported)
    # a multi-bridge dict missing a resident generation: the server's message, the tenant's name in front
    with pytest.raises(ValueError, match=f"tenant 'alice'.*{id1}"):
        hub.rekey("alice", fake_keys(2, bridge_from=[id0]))
    with pytest.raises(ValueError, match=f"tenant 'alice'.*{id0}"):
        hub.rekey("alice", fake_keys(2, bridge_from=[id1, id3]))
    with pytest.raises(ValueError, match="tenant 'alice'.*two generations"):
        hub.rekey("alice", fake_keys(2, bridge_from=id0))
    assert len(s.engine.imported) == n_imp and s.generations == [(id0, 12), (id1, 17)]
    hub.rekey("alice", fake_keys(2, bridge_from=[id0, id1]))
    assert s.old_generations == [(id0, 12), (id1, 17)] and s.key_id == id2 and s.engine.bridge_slots() == [0, 1]
    with pytest.raises(ValueError, match="unknown tenant 'erin'"):
        hub.rekey("erin", fake_keys(2, bridge_from=[id0, id1]))


def test_schedules_hub_hands_every_tenants_row_map_to_the_group(stub_server):  # noqa: F811
    """alice: three old generations (one bridge for a generation that is not
    resident in between, so her slots are not 0, 1, 2); bob: rotated once and
    appended to; carol: never rotated."""
    id0, id1, id2, id3 = ids_of(4)
    hub = make_hub(stub_server, True, ("alice", "bob", "carol"))
    rng = np.random.default_rng(3)
    hub.load("alice", *docs_of(rng, 12))
    hub.rekey("alice", fake_keys(1, bridge_from=id0))
    hub.append("alice", *docs_of(rng, 5))
    hub.rekey("alice", fake_keys(2, bridge_from=[id0, id1]))
    hub.append("alice", *docs_of(rng, 3))
    hub.rekey("alice", fake_keys(3, bridge_from=[id0, "absent", id1, id2]))
    hub.append("alice", *docs_of(rng, 2))
    hub.load("bob", *docs_of(rng, 6))
    hub.rekey("bob", fake_keys(1, bridge_from=id0))
    hub.append("bob", *docs_of(rng, 4))
    hub.load("carol", *docs_of(rng, 7))
    from fheicp.stored import CorpusHub
    assert CorpusHub.gen_map(hub.tenants["alice"]) == ([12, 17, 20], [0, 2, 3])
    assert CorpusHub.gen_map(hub.tenants["bob"]) == ([6], [0])
    assert CorpusHub.gen_map(hub.tenants["carol"]) == ([], [])
    q = np.zeros((2, 16), np.float32)
    requests = {"alice": (q, None), "bob": (q[:1], None), "carol": (q, None)}
    assert [r["mode"] for r in hub.rounds(requests)] == ["group"]
    out = hub.search_many(requests)
    assert [len(out[n]) for n in requests] == [1, 1, 1]
    (entry, items), = hub._group.calls
    assert entry == "gens" and [len(it) for it in items] == [9, 9, 9]
    assert [(it[7], it[8]) for it in items] == [([12, 17, 20], [0, 2, 3]), ([6], [0]), ([], [])]
    assert [int(it[0].shape[0]) for it in items] == [22, 10, 7] and [len(it[5]) for it in items] == [2, 1, 2]
    # a tenant that sits out is None in its place; every group round goes through the new entry
    hub.search_many({"alice": (q, None), "carol": (q, None)})
    entry, items = hub._group.calls[-1]
    assert entry == "gens" and items[1] is None and (items[0][7], items[2][7]) == ([12, 17, 20], [])
    # a tenant alone runs its own server, which handles generations itself
    hub.search_many({"alice": (q, None)})
    assert len(hub._group.calls) == 2
    assert hub.tenants["alice"].engine.searches[-1] == {"B": 22, "ends": [12, 17, 20], "slots": [0, 2, 3], "Q": 2}


@pytest.mark.parametrize("schedules", [None, False])
def test_default_hub_still_calls_the_one_old_generation_entry(stub_server, schedules):  # noqa: F811
    id0, id1 = ids_of(2)
    hub = make_hub(stub_server, schedules, ("bob", "carol"))
    assert hub.rotation_schedules is False
    rng = np.random.default_rng(4)
    hub.load("bob", *docs_of(rng, 6))
    hub.rekey("bob", fake_keys(1, bridge_from=id0))
    hub.append("bob", *docs_of(rng, 4))
    hub.load("carol", *docs_of(rng, 7))
    with pytest.raises(ValueError, match="tenant 'bob'.*one old generation per tenant"):
        hub.rekey("bob", fake_keys(2, bridge_from=[id0, id1]))
    q = np.zeros((2, 16), np.float32)
    hub.search_many({"bob": (q, None), "carol": (q, None)})
    (entry, items), = hub._group.calls
    assert entry == "one" and [len(it) for it in items] == [8, 8] and [it[7] for it in items] == [6, 0]
