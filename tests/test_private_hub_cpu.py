"""CPU: the both-private hub, the parts that need no GPU:
the level-aware chunking, PrivateHub's payload checks on packed-but-fake
payloads, what the two new entries refuse before they look at a group, the
binding's struct against the header, and a numpy restatement of the grouped
row layout that tests/test_gpu_private_hub.py relies on. (A group cannot be
created on host-only contexts, fhe_group_create stops at their missing keys,
so the per-tenant argument checks run in the GPU file.)"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import extprod_ref as X

from fheicp import _lib
from fheicp.params import TOY
from fheicp.private import PrivateServer

E_ARG = -1
U = np.uint64


# ------------------------------------------------------------------ chunking --
def test_chunks_never_mix_gadget_levels():
    from fheicp.private import private_hub_chunks
    sizes = {"a": (1, 128, 6), "b": (2, 128, 6), "c": (1, 128, 7), "d": (3, 128, 6)}
    chunks = private_hub_chunks(sizes)
    assert chunks == [[("a", range(0, 1)), ("b", range(0, 2))], [("c", range(0, 1))], [("d", range(0, 3))]]
    # equal levels: query.hub_chunks's chunks
    from fheicp.query import hub_chunks
    same = {"a": (3, 130, 6), "b": (1, 1, 6), "c": (2, 17, 6)}
    assert private_hub_chunks(same) == hub_chunks({n: s[:2] for n, s in same.items()})
    assert private_hub_chunks({}) == []


@pytest.mark.parametrize("sizes,cap", [
    ({"a": (8, 128, 6), "b": (8, 128, 6), "c": (8, 128, 7), "d": (8, 128, 6)}, 2048),
    ({"a": (5, 100, 3), "b": (7, 33, 3), "c": (0, 4, 5), "d": (3, 1, 3)}, 256),
    ({"a": (2, 9000, 6), "b": (3, 10, 6), "c": (1, 10, 7)}, 8192),
])
def test_chunks_keep_order_cap_and_whole_queries(sizes, cap):
    from fheicp.private import private_hub_chunks
    chunks = private_hub_chunks(sizes, cap)
    bound = max(cap, max(B for _, B, _ in sizes.values()))
    seen = []
    for ch in chunks:
        assert ch and sum(len(r) * sizes[name][1] for name, r in ch) <= bound
        assert len({sizes[name][2] for name, _ in ch}) == 1          # one gadget level per library call
        assert len({name for name, _ in ch}) == len(ch)
        assert all(len(r) > 0 for _, r in ch)
        seen += [(name, q) for name, r in ch for q in r]
    assert seen == [(name, q) for name, (Q, _, _) in sizes.items() for q in range(Q)]


# ------------------------------------------------------------ payload checks --
class StubModel:
    q_w = np.array([2, -1, 2, -2, 1])


class StubQuant:
    model = StubModel()


class StubServer:
    """What PrivateHub reads of a PrivateServer before any device work."""

    def __init__(self, P0, scheme, gadget):
        self.P0, self.scheme, self.cq = P0, scheme, StubQuant()
        self.base_log, self.level = gadget

    def plan(self, min_similarity):
        return None, 0, 0

    _check = PrivateServer._check


def fake_query(D=5, P0=8, gadget=(7, 3), N=TOY.N, k=TOY.k):
    from fheicp.private import pack_ggsw_query
    return pack_ggsw_query(np.zeros((k + 1) * gadget[1] * (k + 1) * N, U), D, P0, *gadget, N, k)


@pytest.fixture()
def hub():
    from fheicp.private import PrivateHub
    h = PrivateHub()
    for name, gadget in (("alice", (7, 3)), ("bob", (7, 3)), ("carol", (5, 4))):
        h.add_tenant(name, None, None, 8, server=StubServer(8, TOY.with_msg_bits(8), gadget))
    h.tenants["alice"].update(docs=object(), B=130)
    h.tenants["bob"].update(docs=object(), B=17)
    return h


def test_private_hub_checks_name_the_tenant(hub):
    ok = fake_query()
    for request, why in (
            ({"alice": ([ok], None), "bob": ([fake_query(gadget=(6, 3))], None)}, "'bob'.*gadget differs"),
            ({"bob": ([ok, fake_query(D=4)], None)}, "'bob'.*query 1: dimension D 4"),
            ({"alice": ([fake_query(P0=12)], None)}, "'alice'.*different parameters"),
            ({"alice": ([ok, ok], [0.5])}, "'alice'.*1 thresholds for 2"),
            ({"alice": ([fake_query(D=4)], None)}, "'alice'.*4 features, the model 5"),
            ({"alice": ([], None)}, "'alice'.*empty batch"),
            ({"alice": ([ok[:-1]], None)}, "'alice'.*size"),
            ({"carol": ([fake_query(gadget=(5, 4))], None)}, "'carol' has no documents"),
            ({"erin": ([ok], None)}, "unknown tenant 'erin'")):
        with pytest.raises(ValueError, match=why):
            hub.search_many(request)


def test_private_hub_refuses_another_p0_by_name(hub):
    with pytest.raises(ValueError, match="'dave'.*P0 = 12"):
        hub.add_tenant("dave", None, None, 12, server=StubServer(12, TOY.with_msg_bits(12), (7, 3)))
    with pytest.raises(ValueError, match="'dave'.*P0 = 12"):                 # before any server is built
        hub.add_tenant("dave", {}, None, 12, scheme=TOY)
    with pytest.raises(ValueError, match="'bob'.*already"):
        hub.add_tenant("bob", None, None, 8, server=StubServer(8, TOY.with_msg_bits(8), (7, 3)))
    from fheicp.query import pack_replies
    n1 = (TOY.k + 1) * TOY.N
    glwes = lambda Q, B: np.zeros(-(-Q * B // TOY.N) * n1, dtype=U)  # noqa: E731
    assert hub.check_reply("alice", pack_replies(glwes(3, 130), glwes(3, 130), 130, 8, [0, 1, 2]), 3)["Q"] == 3
    with pytest.raises(ValueError, match="'bob'.*130 documents"):
        hub.check_reply("bob", pack_replies(glwes(3, 130), glwes(3, 130), 130, 8, [0, 1, 2]), 3)
    hub.close()


# ------------------------------------------------------------------- the ABI --
def test_new_entries_reject_a_null_group():
    L = _lib.lib()
    arr = (_lib.FheGroupGgsw * 1)()
    assert L.fhe_linear_ggsws_group_batch(None, arr, 1, None, None, None) == E_ARG
    assert b"group" in L.fhe_last_error(None)
    assert L.fhe_search_ggsws_group_batch(None, arr, 1, None) == E_ARG
    assert b"group" in L.fhe_last_error(None)


def test_binding_struct_is_the_headers():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "fhe_icp.h").read_text()
    body = re.search(r"typedef struct fhe_group_ggsw \{(.*?)\} fhe_group_ggsw;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f for f, _ in _lib.FheGroupGgsw._fields_] and fields[0] == "struct_size"
    assert {"d_ggsw", "base_log", "level", "d_docs", "Q", "B", "D", "cst", "h_T", "levels_bit", "d_glwe_acc",
            "d_glwe_bit", "reserved"} == set(fields[1:])
    assert C.sizeof(_lib.FheGroupGgsw) == 88
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for name, nargs in (("fhe_linear_ggsws_group_batch", 6), ("fhe_search_ggsws_group_batch", 4)):
        decl = re.search(name + r"\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)
        assert len(decl.group(1).split(",")) == nargs == len(bound[name]), name


# ------------------------------------------------------- the grouped layout --
def test_grouped_layout_restatement():
    """What fhe_linear_ggsws_group_batch writes, restated: tenant t's Q_t B_t
    rows (query-major, each extprod_ref's slot extraction of its own product
    with its own constant) at fhe_group_rows' start_t; the rows between
    start_t + Q_t B_t and the next start are padding."""
    from fheicp.engine import group_rows
    N, k, beta, Lv, P = 256, 2, 4, 2, 8
    rng = np.random.default_rng(5)
    specs = [(2, 1, 16), None, (1, 2, 128), (3, 1, 256)]          # (Q, G, D); a tenant sitting out
    tenants, counts = [], []
    for s in specs:
        if s is None:
            tenants.append(None)
            counts.append(0)
            continue
        Qn, G, D = s
        S = N // D
        B = G * S if S == 1 else (G - 1) * S + max(1, S // 3)
        glwe = rng.integers(0, 2 ** 64, (G, k + 1, N), dtype=U)
        rows = []
        for q in range(Qn):
            ggsw = rng.integers(0, 2 ** 64, (k + 1, Lv, k + 1, N), dtype=U)
            rows.append(X.extract_slots(X.external_product(glwe, ggsw, beta), B, D, ((7 - q) << (64 - P)) % 2 ** 64))
        tenants.append(np.concatenate(rows))
        counts.append(Qn * B)
    assert counts == [10, 0, 3, 3]
    M, starts = group_rows(counts)
    assert (M, starts) == (20, [0, 12, 12, 16])
    SENT = U(0x5EA15EA15EA15EA1)
    out = np.full((M, k * N + 1), SENT, U)
    for rows, st in zip(tenants, starts):
        if rows is not None:
            out[st:st + len(rows)] = rows
    padding = [r for r in range(M) if (out[r] == SENT).all()]
    assert padding == [10, 11, 15, 19]
    # query-major within a tenant: tenant 0's row q B + b is document b under query q
    B0 = counts[0] // 2
    np.testing.assert_array_equal(out[B0:2 * B0], tenants[0][B0:])
    assert (out[0] != out[B0]).any()
