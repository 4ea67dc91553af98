"""CPU: several key holders in one batched call, the parts
that need no GPU: the padded row layout (fhe_group_rows), the checks of
fhe_group_create in their order on host-only contexts, and QueryHub's pure
Python: the shared-P0 check, the chunking and the per-tenant reply check."""
import ctypes as C

import numpy as np
import pytest

from fheicp import _lib
from fheicp.params import TOY, params_for_bits

E_ARG, E_STATE = -1, -3


def rows(counts):
    L = _lib.lib()
    n = len(counts)
    c = (C.c_int64 * n)(*counts)
    s = (C.c_int64 * n)()
    return L.fhe_group_rows(c, n, s), tuple(s)


def test_group_rows_layout():
    assert rows((5, 1, 6)) == (20, (0, 8, 12))
    assert rows((4, 0, 1)) == (8, (0, 4, 4))
    assert rows((0, 0, 0)) == (0, (0, 0, 0))
    assert rows((1, 1, 1)) == (12, (0, 4, 8))
    assert rows((3, -1))[0] == -1
    assert _lib.lib().fhe_group_rows(None, 2, None) == -1
    from fheicp.engine import group_rows
    assert group_rows([5, 1, 6]) == (20, [0, 8, 12])


@pytest.fixture()
def host_ctx():
    """make(params) -> a host-only context, destroyed after the test."""
    L = _lib.lib()
    made = []

    def make(p):
        h = C.c_void_p()
        assert L.fhe_ctx_create(C.byref(_lib.params_struct(p.as_dict())), -1, C.byref(h)) == 0
        made.append(h)
        return h
    yield make
    for h in made:
        L.fhe_ctx_destroy(h)


def create(ctxs, T=None):
    L = _lib.lib()
    n = len(ctxs)
    arr = (C.c_void_p * max(n, 1))(*[c.value if c is not None else None for c in ctxs])
    g = C.c_void_p()
    rc = L.fhe_group_create(arr, n if T is None else T, C.byref(g))
    msg = L.fhe_last_error(None)
    if rc == 0:
        L.fhe_group_destroy(g)
    else:
        assert not g.value
    return rc, msg


def test_group_create_argument_checks(host_ctx):
    a, b = host_ctx(TOY), host_ctx(TOY)
    for ctxs, T in (([a], 0), ([a] * 65, 65), ([a, None], 2), ([a, b, a], 3)):
        rc, msg = create(ctxs, T)
        assert rc == E_ARG and b"group" in msg, (T, msg)
    rc, msg = create([a, None])
    assert b"null" in msg
    rc, msg = create([a, b, a])
    assert b"repeats" in msg


def test_group_create_parameter_checks(host_ctx):
    a, b = host_ctx(TOY), host_ctx(TOY)
    rc, msg = create([a, host_ctx(TOY.with_msg_bits(12)), b])
    assert rc == E_ARG and b"group" in msg and b"tenant 1" in msg, msg
    # the differing tenant is named by its index, not by its place after tenant 0
    rc, msg = create([a, b, host_ctx(TOY.with_msg_bits(12))])
    assert rc == E_ARG and b"tenant 2" in msg, msg
    # P = 27 has a classic round on the N = 1024 kernels: no group form
    rc, msg = create([host_ctx(params_for_bits(27)), host_ctx(params_for_bits(27))])
    assert rc == E_ARG and b"group" in msg and b"classic" in msg, msg
    # the parameter check comes first: a differing set is reported before the schedule
    rc, msg = create([host_ctx(params_for_bits(27)), host_ctx(params_for_bits(26))])
    assert rc == E_ARG and b"tenant 1" in msg, msg


def test_group_create_reaches_the_key_check(host_ctx):
    """Valid host-only contexts pass the argument, parameter and schedule
    checks and stop at the key check: every planned set from P = 4 to 26 and
    TOY has a group kernel for every round."""
    rc, msg = create([host_ctx(TOY), host_ctx(TOY)])
    assert rc == E_STATE and b"group" in msg and b"keys" in msg, msg
    for P in range(4, 27):
        p = params_for_bits(P)
        rc, msg = create([host_ctx(p), host_ctx(p)])
        assert rc == E_STATE, (P, msg)
    rc, msg = create([host_ctx(TOY)])                      # T = 1 is a group too
    assert rc == E_STATE


def test_group_calls_reject_null_group():
    L = _lib.lib()
    c = (C.c_int64 * 1)(1)
    assert L.fhe_sign_group_batch(None, None, c, None, None) == E_ARG
    assert b"group" in L.fhe_last_error(None)
    assert L.fhe_search_query_group_batch(None, None, 1, None) == E_ARG
    L.fhe_group_destroy(None)
    # the binding's struct is the header's: struct_size leads, 13 more fields
    import re
    from pathlib import Path
    hdr = (Path(__file__).resolve().parents[1] / "include" / "fhe_icp.h").read_text()
    body = re.search(r"typedef struct fhe_group_query \{(.*?)\} fhe_group_query;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f for f, _ in _lib.FheGroupQuery._fields_] and fields[0] == "struct_size"
    assert C.sizeof(_lib.FheGroupQuery) == 104


# ------------------------------------------------------------------ QueryHub --
class StubServer:
    def __init__(self, P0, scheme):
        self.P0, self.scheme = P0, scheme


def test_hub_refuses_another_p0_by_name():
    from fheicp.query import QueryHub
    hub = QueryHub()
    hub.add_tenant("alice", None, None, 8, server=StubServer(8, TOY))
    hub.add_tenant("bob", None, None, 8, server=StubServer(8, TOY))
    with pytest.raises(ValueError, match="'carol'.*P0 = 12"):
        hub.add_tenant("carol", None, None, 12, server=StubServer(12, TOY.with_msg_bits(12)))
    # refused before any server is built from the keys (there is no GPU here)
    with pytest.raises(ValueError, match="'carol'.*P0 = 12"):
        hub.add_tenant("carol", {}, None, 12, scheme=TOY)
    with pytest.raises(ValueError, match="'dave'.*scheme"):
        hub.add_tenant("dave", None, None, 8, server=StubServer(8, params_for_bits(8)))
    with pytest.raises(ValueError, match="'bob'.*already"):
        hub.add_tenant("bob", None, None, 8, server=StubServer(8, TOY))
    assert list(hub.tenants) == ["alice", "bob"]
    with pytest.raises(ValueError, match="unknown tenant 'erin'"):
        hub.search_many({"erin": ([], None)})


@pytest.mark.parametrize("sizes,cap", [
    ({"a": (3, 130), "b": (1, 1), "c": (2, 17)}, 8192),          # one chunk
    ({"a": (8, 128), "b": (8, 128), "c": (8, 128)}, 2048),       # whole tenants per chunk, then a split one
    ({"a": (5, 100), "b": (7, 33), "c": (0, 4), "d": (3, 1)}, 256),
    ({"a": (2, 9000), "b": (3, 10)}, 8192),                      # B above the cap: one query per chunk
    ({"a": (70, 130), "b": (1, 8192), "c": (1, 1)}, 8192),
])
def test_hub_chunks_cover_every_query_once_within_the_cap(sizes, cap):
    from fheicp.query import hub_chunks
    chunks = hub_chunks(sizes, cap)
    bound = max(cap, max(B for _, B in sizes.values()))
    seen = []
    for ch in chunks:
        assert ch and sum(len(r) * sizes[name][1] for name, r in ch) <= bound
        assert len({name for name, _ in ch}) == len(ch)          # one piece per tenant and chunk
        assert all(len(r) > 0 for _, r in ch)
        seen += [(name, q) for name, r in ch for q in r]
    want = [(name, q) for name, (Q, _) in sizes.items() for q in range(Q)]
    assert seen == want                                           # once each, tenants and queries in order


def test_hub_chunks_shapes():
    from fheicp.query import hub_chunks
    assert hub_chunks({"a": (3, 130), "b": (1, 1), "c": (2, 17)}) == [[("a", range(0, 3)), ("b", range(0, 1)),
                                                                      ("c", range(0, 2))]]
    # 8 tenants x (Q = 1, B = 128): one group call
    assert len(hub_chunks({t: (1, 128) for t in range(8)})) == 1
    assert hub_chunks({"a": (2, 9000), "b": (1, 10)}) == [[("a", range(0, 1))], [("a", range(1, 2))],
                                                           [("b", range(0, 1))]]
    assert hub_chunks({}) == [] and hub_chunks({"a": (0, 5)}) == []
    with pytest.raises(ValueError):
        hub_chunks({"a": (1, 0)})


def test_hub_reply_to_the_wrong_tenant_raises():
    from fheicp.query import QueryHub, pack_replies
    hub = QueryHub()
    for name, B in (("alice", 130), ("bob", 17)):
        hub.add_tenant(name, None, None, 8, server=StubServer(8, TOY))
        hub.tenants[name]["B"] = B
    n1 = (TOY.k + 1) * TOY.N
    glwes = lambda Q, B: np.zeros(-(-Q * B // TOY.N) * n1, dtype=np.uint64)  # noqa: E731
    to_alice = pack_replies(glwes(3, 130), glwes(3, 130), 130, 8, [0, 1, 2])
    to_bob = pack_replies(glwes(2, 17), glwes(2, 17), 17, 8, [5, 6])
    assert hub.check_reply("alice", to_alice, 3)["Q"] == 3
    assert hub.check_reply("bob", to_bob, 2)["B"] == 17
    with pytest.raises(ValueError, match="'bob'.*130 documents"):
        hub.check_reply("bob", to_alice, 3)
    with pytest.raises(ValueError, match="'alice'"):
        hub.check_reply("alice", to_bob, 2)
    with pytest.raises(ValueError, match="'alice'"):
        hub.check_reply("alice", to_alice, 2)                     # another call's query count
    with pytest.raises(ValueError, match="size"):
        hub.check_reply("alice", to_alice[:-n1], 3)
    with pytest.raises(ValueError, match="P0 = 12"):
        hub.check_reply("alice", pack_replies(glwes(3, 130), glwes(3, 130), 130, 12, [0, 1, 2]), 3)
