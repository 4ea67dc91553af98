"""CPU: several private queries in one batched call (DESIGN.md §8.8,
fheicp.query) — the version-2 reply, the payload-batch checks, the chunking
rule, the new entry points' validation on a host-only context, and the three
places that mirror the C ABI."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from fheicp import _lib
from fheicp.params import params_for_bits
from fheicp.query import (REPLY_HEADER_WORDS, REPLY_MAGIC, check_query_batch, pack_query, pack_replies, pack_reply,
                          query_chunks, thresholds_for, unpack_query, unpack_replies, unpack_reply)

REPO = Path(__file__).resolve().parents[1]
NEW = ("fhe_linear_queries_batch", "fhe_compare_queries_batch", "fhe_search_queries_batch")
N, N1 = 256, 768   # TOY: N, (k+1)N


def test_reply_v2_round_trip_and_errors():
    Q, B, P0 = 3, 130, 8
    G = -(-(Q * B) // N)
    assert G == 2
    ga = np.arange(G * N1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    gb = ga[::-1].copy()
    Ts = [-35, 0, 17]
    r = pack_replies(ga, gb, B, P0, Ts)
    assert r.dtype == np.uint64 and r.size == REPLY_HEADER_WORDS + Q + 2 * G * N1
    assert int(r[0]) == REPLY_MAGIC and int(r[1]) == 2 | (P0 << 32) and (int(r[2]), int(r[3])) == (B, Q)
    u = unpack_replies(r, N1, N)
    assert (u["P0"], u["B"], u["Q"], u["T"]) == (P0, B, Q, Ts)
    np.testing.assert_array_equal(u["glwe_acc"], ga)
    np.testing.assert_array_equal(u["glwe_bit"], gb)
    # without the scheme's sizes the split is still the halves
    np.testing.assert_array_equal(unpack_replies(r)["glwe_bit"], gb)
    # a size that does not match ceil(Q B / N) GLWEs per block: one GLWE short, one too many
    for bad in (pack_replies(ga[:N1], gb[:N1], B, P0, Ts), pack_replies(np.tile(ga, 2)[:3 * N1], np.tile(gb, 2)[:3 * N1],
                                                                         B, P0, Ts)):
        with pytest.raises(ValueError, match="size"):
            unpack_replies(bad, N1, N)
    with pytest.raises(ValueError, match="odd"):
        unpack_replies(r[:-1], N1, N)
    with pytest.raises(ValueError):
        unpack_replies(r[:REPLY_HEADER_WORDS + Q - 1])            # the thresholds are cut
    with pytest.raises(ValueError):
        unpack_replies(r.astype(np.int64))
    v = r.copy()
    v[1] = np.uint64(3 | (P0 << 32))
    with pytest.raises(ValueError, match="version 3"):
        unpack_replies(v)
    # the two versions do not read each other
    with pytest.raises(ValueError, match="version 2"):
        unpack_reply(r)
    r1 = pack_reply(ga[:N1], gb[:N1], 40, 21, -5)
    with pytest.raises(ValueError, match="version 1"):
        unpack_replies(r1)


def test_reply_v1_still_unpacks():
    ga = np.arange(N1, dtype=np.uint64)
    r1 = pack_reply(ga, ga + np.uint64(1), 40, 21, -5)
    assert r1.size == 4 + 2 * N1 and int(r1[1]) == 1 | (21 << 32)
    u = unpack_reply(r1)
    assert (u["P0"], u["B"], u["T"]) == (21, 40, -5)
    np.testing.assert_array_equal(u["glwe_acc"], ga)
    np.testing.assert_array_equal(u["glwe_bit"], ga + np.uint64(1))


def payloads(ids, D=16, P0=21, key=None, big=2048):
    key = np.arange(8, dtype=np.uint32) + 5 if key is None else key
    return [unpack_query(pack_query(np.zeros(D, np.uint64), i, P0, key, big)) for i in ids]


def test_payload_batch_checks_name_the_query():
    check_query_batch(payloads([0, 16, 32, 2 ** 64 - 16]))         # touching ranges, the last ends at 2^64
    check_query_batch(payloads([7]))
    check_query_batch(payloads([100, 0, 50]))                      # any order
    with pytest.raises(ValueError, match="empty"):
        check_query_batch([])
    good = payloads([0, 100, 200])
    for field, other in (("P0", payloads([300], P0=20)), ("D", payloads([300], D=15)),
                         ("big", payloads([300], big=1024)),
                         ("mask", payloads([300], key=np.arange(8, dtype=np.uint32)))):
        with pytest.raises(ValueError, match="query 2"):
            check_query_batch(good[:2] + other + good[2:])
    # overlaps: equal ids, a partial overlap, and a range that wraps 2^64 onto query 0's
    with pytest.raises(ValueError, match="query 1.*overlap"):
        check_query_batch(payloads([5, 5]))
    with pytest.raises(ValueError, match="query 2.*overlap query 0"):
        check_query_batch(payloads([100, 300, 115]))
    with pytest.raises(ValueError, match="query 3.*overlap query 0"):
        check_query_batch(payloads([3, 100, 200, 2 ** 64 - 10]))
    with pytest.raises(ValueError, match="query 1.*overlap query 0"):
        check_query_batch(payloads([2 ** 64 - 1, 2 ** 64 - 16]))
    check_query_batch(payloads([0, 100, 200, 2 ** 64 - 16]))


def test_query_chunks():
    for Q, B, cap in ((8, 128, 8192), (65, 128, 8192), (64, 128, 8192), (5, 8192, 8192), (5, 8193, 8192),
                      (3, 20000, 8192), (7, 3, 10), (1, 1, 8192), (0, 4, 8192), (9000, 1, 8192)):
        ch = query_chunks(Q, B, cap)
        assert all(isinstance(c, range) for c in ch)
        assert [q for c in ch for q in c] == list(range(Q)), (Q, B, cap)
        assert all(1 <= len(c) and len(c) * B <= max(B, cap) for c in ch), (Q, B, cap)
        if B > cap:
            assert [len(c) for c in ch] == [1] * Q
    assert query_chunks(8, 128) == [range(0, 8)]
    assert query_chunks(65, 128) == [range(0, 64), range(64, 65)]
    assert query_chunks(7, 3, 10) == [range(0, 3), range(3, 6), range(6, 7)]
    with pytest.raises(ValueError):
        query_chunks(4, 0)


def test_thresholds_for():
    assert thresholds_for(0.5, 3) == [0.5] * 3 and thresholds_for(None, 2) == [None, None]
    assert thresholds_for([0.1, None, 0.3], 3) == [0.1, None, 0.3]
    assert thresholds_for(np.float64(0.25), 2) == [0.25, 0.25]
    with pytest.raises(ValueError, match="2 thresholds for 3"):
        thresholds_for([0.1, 0.2], 3)


def test_new_exports_present_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fhe_icp.h").read_text(), flags=re.S)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    integ = (REPO / "integration" / "fhe_gpu.py").read_text()
    guide = (REPO / "INTEGRATION.md").read_text()
    L = _lib.lib()
    for name in NEW:
        m = re.search(r"^int " + name + r"\((.*?)\);", hdr, flags=re.S | re.M)
        assert m, name
        assert len(bound[name]) == m.group(1).count(",") + 1, name    # one ctypes argument per C parameter
        assert hasattr(L, name)
        assert f'"{name}"' in integ and name in guide
    # appended: the new declarations follow everything the header had
    assert hdr.index("fhe_build_info") < min(hdr.index(n) for n in NEW)
    for meth in ("compare_many", "encrypt_queries", "search_many", "decrypt_replies"):
        assert f"def {meth}" in (REPO / "fhe-icp_amd" / "fheicp" / "query.py").read_text()
    from batch_operations import BatchProcessor
    assert callable(BatchProcessor.search_vectors) and callable(BatchProcessor.search_similar_many)


def test_queries_entry_points_on_host_context():
    """Argument errors first (FHE_E_ARG, a host-only context reports them
    too), then the missing device; Q < 1, B < 1 and D outside (0, 65536]."""
    L = _lib.lib()
    P = _lib.params_struct(params_for_bits(16).as_dict())
    h = C.c_void_p()
    assert L.fhe_ctx_create(C.byref(P), -1, C.byref(h)) == 0
    key = (C.c_uint32 * 8)()
    lin = lambda Q, B, D: L.fhe_linear_queries_batch(h, None, Q, None, B, D, None, None, None, None)  # noqa: E731
    cmp_ = lambda Q, B, D: L.fhe_compare_queries_batch(h, None, None, key, Q, None, B, D, None, 0, None, None,  # noqa: E731
                                                       None, None)
    sea = lambda Q, B, D, lb=0: L.fhe_search_queries_batch(h, None, None, key, Q, None, B, D, None, 0, None,  # noqa: E731
                                                           lb, None, None, None)
    for f in (lin, cmp_, sea):
        for Q, B, D in ((0, 4, 16), (-1, 4, 16), (2, 0, 16), (2, -3, 16), (2, 4, 0), (2, 4, 65537), (65536, 4, 16)):
            assert f(Q, B, D) == -1, (Q, B, D)
            assert b"queries" in L.fhe_last_error(h)
        assert f(2, 4, 16) == -2
        assert b"host-only" in L.fhe_last_error(h)
    assert sea(2, 4, 16, 9) == -1 and sea(2, 4, 16, -1) == -1
    assert L.fhe_linear_queries_batch(None, None, 1, None, 1, 1, None, None, None, None) == -1
    L.fhe_ctx_destroy(h)
