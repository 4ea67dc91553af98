#!/usr/bin/env python3
"""Private-query search: the leveled step against the seeded-corpus one, and
the end-to-end compare rate (docs/AB_LOG_r07.md).

For B = 1024 documents at D = 16 and D = 768 (C2's and C5's dimensions) and
n_bits 6 and 8, in one process:

  * the "linear_query" profile bucket (fhe_linear_query_batch: query byte
    planes + the i8 MFMA GEMM, one HIP-event bracket around both) and
    fhe_linear_seeded_batch at the same B and D (HIP events around the call),
    interleaved launch by launch, the median of --launches launches each
    after --warmup;
  * fhe_compare_query_batch end to end (host clock around the call and a
    device synchronise) as compares/s, its accumulators checked against the
    oracle restatement. A shape whose worst-case width P0 has no parameter
    set (P0 > 27) reports null there.

With --two-party (docs/AB_LOG_r08.md) it measures the two-party
search instead: QueryServer.search on an evaluation-only context (host clock
around the call: expansion, GEMM, sign extraction, both packings and the
reply's copy to the host) interleaved step by step, in alternating order,
with fhe_compare_query_batch on the key holder's context; the "pack" profile
bucket per search, the reply's size, and the parity of the client's decrypted
(acc, below) with the single-party result.

With --both-private (docs/AB_LOG_r09.md) it measures the
both-private compare: fhe_compare_ggsw_batch (a GGSW query against packed GLWE
documents; payload parse and upload, Toeplitz planes, GEMM, slot extraction,
sign extraction, both decryptions) interleaved step by step, in alternating
order, with fhe_compare_query_batch on the same context, the "linear_ggsw"
profile bucket per compare, and the parity of the two results.

With --multi-query (docs/AB_LOG_r11.md) it measures several
queries in one batched call, two-party, at 16 dimensions, n_bits 6 (P0 = 21):
QueryServer.search_many with Q = 8, B = 128 against eight sequential
QueryServer.search calls at B = 128 and one at B = 1024, 24 steps after 4
warm-up in rotating order, with the "linear_query" and "blind_rotate"
buckets and the reply bytes of each; it writes profiles/r11/multi_query.json.

With --stored-queries (docs/AB_LOG_r12.md) it measures the
stored-ciphertext search for several clear queries, two-party, at 16
dimensions, n_bits 6 (P0 = 21): CorpusServer.search_many with Q = 8, B = 128
against eight sequential CorpusServer.search calls at B = 128 and one
EncryptedCorpus.compare at B = 1024, 24 steps after 4 warm-up in rotating
order; then the "linear_seeded" bucket of the batched leveled step against
HIP events around eight fhe_linear_seeded_batch calls on the same documents at
B = 128 and B = 1024, with the outputs compared; it writes
profiles/r12/stored_queries.json (--no-end-to-end: the leveled step only).

With --private-queries (docs/AB_LOG_r13.md) it measures the
both-private search for several GGSW queries, two-party, at 16 dimensions,
n_bits 6 (P0 = 21): PrivateServer.search_many with Q = 8, B = 128 against
eight sequential PrivateServer.search calls at B = 128 and one at B = 1024, 24
steps after 4 warm-up in rotating order; then the "linear_ggsws" bucket of the
batched leveled step against HIP events around eight fhe_linear_ggsw_batch
calls on the same documents at B = 128 and B = 1024, with the outputs
compared, and the same at Q = 1; it writes profiles/r13/private_queries.json
(--no-end-to-end: the leveled step only, gadget (7, 6)).

With --tenants (docs/AB_LOG_r14.md) it measures several key
holders in one batched call, two-party, at 16 dimensions, n_bits 6 (P0 = 21):
QueryHub.search_many for 8 tenants x (Q = 1, B = 128), each with its own keys
and documents, against the eight QueryServer.search calls one after another
and one tenant's search at B = 1024, 24 steps after 4 warm-up in rotating
order, with the HIP-event split of each (rotations, key switches, leveled
step, packings: the profile buckets summed over the tenants' contexts); it
writes profiles/r14/tenants.json (--tenant-shape T B: another shape).

With --rotated (docs/AB_LOG_r15.md) it measures the
stored-ciphertext search after a key rotation, two-party, at 16 dimensions,
n_bits 6 (P0 = 21): CorpusServer.search_many on a server holding the new
generation's keys and bridge key, at 8 queries x 128 documents and 1 x 1024,
with every, half and none of the documents old-generation, 24 steps after 4
warm-up in rotating order, then the "bridge" and "pack" buckets of each leg
and its parity with the restatement; it writes profiles/r15/rotated.json.
With --generations G > 1 (docs/AB_LOG_r20.md) the server holds
a direct bridge key from each of G old generations and the legs are "the G old
generations in equal parts" (the generation row map, one grouped bridge), "all
documents of one old generation" (the single bridge over the same rows) and
"none old"; it reports the "bridge" bucket per leg (three rounds of five
searches) and writes profiles/r20/rotated_gens.json. FHEICP_LIB selects the
-DFHEICP_GRP_BRIDGE=0 build (tools/build_variant.sh) for the A/B.

With --stored-tenants (docs/AB_LOG_r16.md) it measures
several key holders' STORED documents in one batched call, two-party, at 16
dimensions, n_bits 6 (P0 = 21): CorpusHub.search_many for 8 tenants x (Q = 1,
B = 128 stored documents) against the eight CorpusServer.search calls one
after another and one tenant's 1 x 1024 search, 24 steps after 4 warm-up in
rotating order, with the HIP-event split of each (rotations, key switches,
bridge, packings, leveled step), then a second pass with every tenant rotated
(all documents old-generation); it writes profiles/r16/stored_tenants.json.
With --generations G (docs/AB_LOG_r21.md) every tenant's
documents lie in G old generations in equal parts and none current, 8 queries
per tenant; CorpusHub(rotation_schedules=True) (one grouped bridge pass over
all tenants' generations) is timed and, at G = 1, alternates with the default
hub (one single-key bridge per tenant) in one process; it reports the search
time and the "bridge" bucket per hub search and writes
profiles/r21/stored_tenants_gens.json.

With --private-tenants (docs/AB_LOG_r17.md) it measures
several key holders' BOTH-PRIVATE searches in one batched call, two-party, at
16 dimensions, n_bits 6 (P0 = 21, gadget (7, 6)): PrivateHub.search_many for 8
tenants x (Q = 1, B = 128 encrypted documents) against the eight
PrivateServer.search calls one after another and one tenant's 1 x 1024 search,
24 steps after 4 warm-up in rotating order, with the HIP-event split of each;
then the grouped leveled step's "linear_ggsws" bucket against the sum of the
tenants' own fhe_linear_ggsws_batch calls on the same operands (outputs
compared), at the tenant shape and at 2 x 512; it writes
profiles/r17/private_tenants.json.

With --seeded-private (docs/AB_LOG_r18.md) it measures the
both-private search on seeded payloads against the full form at 16 dimensions,
n_bits 6 (P0 = 21, gadget (7, 6)), one process, one evaluation-only server:
the payload bytes; PrivateServer.pack_docs_many (parse, host-to-device copy,
operand kernel) at B = 1024 and B = 65536 with the operand step alone on
resident inputs; PrivateServer.search_many for 8 queries x 128 documents,
seeded between two full-form series, 24 steps after 4 warm-up in rotating
order; and k_expand_ggsw_seeded alone. The two clients' ciphertext words
coincide, so operands and replies are compared word for word; it writes
profiles/r18/seeded_private.json.

With --seeded-keys (docs/AB_LOG_r19.md) it measures seeded
evaluation keys against the full form at 16 dimensions, n_bits 6 (P0 = 21):
the bytes of both forms of one client's key set, array by array;
Engine.import_eval_keys (host arrays in, context ready) for each form on one
evaluation-only context, interleaved in alternating order after warm-up; and
one search on a QueryServer, a CorpusServer and a PrivateServer built from the
seeded dict against servers built from the full form of the same keys, the
replies compared word for word and decrypted against the clear restatement.
No threshold: the feature's case is size. It writes
profiles/r19/seeded_keys.json.

The floor of the leveled step is its output, B * (kN + 1) * 8 bytes, over the
6.29 TB/s a float4 copy reaches on the MI355X; `floor_fraction` is that floor
over the measured time. Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO / "fhe-icp_amd"), str(REPO)):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_BW = 6.29e12  # bytes/s, measured float4 copy on the MI355X
MAX_BITS = 27      # widest accumulator params_for_bits plans


def corpus_quant(D: int, n_bits: int):
    import numpy as np
    from oracle import quant_ref as Q
    from fheicp.corpus import CorpusQuant
    from fheicp.datagen import training_embeddings
    from fheicp.model import FheLinearModel
    X, y = Q.prepare_training_data(D, 1000, seed=1236)
    m = FheLinearModel.fit(X, y, n_bits)
    e1, e2 = training_embeddings(D, 1000, seed=0)
    return CorpusQuant.calibrate(m.qparams, np.concatenate([e1, e2])), Q.fit_quantized_linear(X, y, n_bits)


def leveled(eng, B: int, D: int, n_bits: int, launches: int, warmup: int) -> dict:
    """Interleaved medians (ms) of the linear_query bucket and fhe_linear_seeded_batch."""
    import numpy as np
    import torch
    rng = np.random.default_rng(D * 100 + n_bits)
    u64 = lambda shape: eng.to_dev(rng.integers(0, 2 ** 64, shape, dtype=np.uint64))  # noqa: E731
    ct_q, body, ids = u64((D, eng.W)), u64((B, D)), u64(B)
    dq = eng.to_dev(rng.integers(-(2 ** (n_bits - 1)), 2 ** (n_bits - 1), (B, D)))
    docs8 = eng.pack_docs(dq)
    w = eng.to_dev(rng.integers(-(2 ** (n_bits - 1)), 2 ** (n_bits - 1), D))
    mk = eng.key_from_seed(11)
    eng.profile(True)
    t_q, t_s = [], []
    for i in range(warmup + launches):
        eng.linear_query(ct_q, docs8, B, D, w, 3)
        r = eng.profile_read("linear_query")
        assert r["launches"] == 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.linear_seeded(body, ids, mk, w, 3)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            t_q.append(r["total_ms"])
            t_s.append(e0.elapsed_time(e1))
    eng.profile(False)
    q_ms, s_ms = statistics.median(t_q), statistics.median(t_s)
    out_bytes = B * eng.W * 8
    floor_ms = out_bytes / COPY_BW * 1e3
    return {"linear_query_ms": q_ms, "linear_query_min_ms": min(t_q), "linear_seeded_ms": s_ms,
            "linear_seeded_min_ms": min(t_s), "ratio_query_over_seeded": q_ms / s_ms, "launches": launches,
            "kernel": eng.kernel_name("linear_query"), "out_bytes": out_bytes, "floor_ms": floor_ms,
            "floor_fraction": floor_ms / q_ms}


def end_to_end(cq, oq, B: int, D: int, n_bits: int, reps: int) -> dict:
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.query import EncryptedQuerySearch
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    qs = EncryptedQuerySearch(c)
    q, docs = Q.make_corpus(D, B, seed=21)
    docs8 = qs.pack_docs(docs)
    payload = qs.encrypt_query(q)
    times = []
    for i in range(reps + 1):   # the first call warms up (workspace, code objects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc, below = qs.compare(payload, docs8, B, 0.5)
        torch.cuda.synchronize()
        if i:
            times.append(time.perf_counter() - t0)
    ref = Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs)
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    exact = bool(np.array_equal(acc.cpu().numpy(), ref) and
                 np.array_equal(below.cpu().numpy(), (scores < 0.5).astype(np.int64)))
    sec = statistics.median(times)
    from fheicp.params import sign_pbs_count
    c.engine.close()
    return {"compare_query_ms": sec * 1e3, "compares_per_s": B / sec, "reps": reps, "bit_exact": exact,
            "pbs_per_compare": sign_pbs_count(c.scheme)}


def two_party(cq, oq, B: int, D: int, n_bits: int, steps: int, warmup: int) -> dict:
    """Server search (evaluation keys only, packed reply) against the
    single-party compare, interleaved in alternating order."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.query import EncryptedQuerySearch, QueryClient, QueryServer
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    single = EncryptedQuerySearch(c)
    client = QueryClient(c, count=B, pack_seed=17)
    server = QueryServer(client.eval_keys(), cq, c.P0)
    q, docs = Q.make_corpus(D, B, seed=21)
    docs8_c, docs8_s = single.pack_docs(docs), server.pack_docs(docs)
    payload = client.encrypt_query(q)
    server.engine.profile(True)
    t_single, t_server, t_pack = [], [], []

    def run_single():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = single.compare(payload, docs8_c, B, 0.5)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def run_server():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = server.search(payload, docs8_s, B, 0.5)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for i in range(warmup + steps):
        if i % 2:
            (ts, res), (tv, reply) = run_single(), run_server()
        else:
            (tv, reply), (ts, res) = run_server(), run_single()
        pk = server.engine.profile_read("pack")
        assert pk["launches"] == 2
        if i >= warmup:
            t_single.append(ts)
            t_server.append(tv)
            t_pack.append(pk["total_ms"])
    server.engine.profile(False)
    acc, below = client.decrypt_reply(reply)
    ref = Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs)
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    parity = bool(torch.equal(acc, res[0]) and torch.equal(below, res[1]))
    exact = bool(np.array_equal(acc.cpu().numpy(), ref) and
                 np.array_equal(below.cpu().numpy(), (scores < 0.5).astype(np.int64)))
    s_ms, v_ms = statistics.median(t_single) * 1e3, statistics.median(t_server) * 1e3
    p = c.scheme
    out = {"server_search_ms": v_ms, "server_search_min_ms": min(t_server) * 1e3, "compare_query_ms": s_ms,
           "compare_query_min_ms": min(t_single) * 1e3, "ratio_server_over_compare": v_ms / s_ms,
           "meets_bar": v_ms <= 1.10 * s_ms, "pack_ms_per_search": statistics.median(t_pack),
           "pack_kernel": server.engine.kernel_name("pack"), "pack_gadget": [client.base_log, client.level],
           "pack_bit_levels": client.bit_levels, "pack_margin_sigmas": client.margin,
           "reply_bytes": int(reply.nbytes), "unpacked_reply_bytes": 2 * B * (p.k * p.N + 1) * 8,
           "parity_with_compare_query": parity, "bit_exact": exact, "steps": steps, "warmup": warmup}
    server.engine.close()
    c.engine.close()
    return out


def multi_query(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Qn: int = 8, B: int = 128,
                B_full: int = 1024) -> dict:
    """Two-party, one process, three things interleaved in rotating order:
    (a) QueryServer.search_many with Qn queries against B documents, (b) Qn
    sequential QueryServer.search calls against the same B documents, (c) one
    QueryServer.search against B_full = Qn * B documents (the same ciphertext
    count as (a)). Host clock around each (reply copies included), the
    "linear_query" and "blind_rotate" profile buckets per run, reply bytes,
    and the parity of (a)'s decrypted reply with (b)'s and the restatement."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.query import QueryClient, QueryServer
    assert Qn * B == B_full
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    client = QueryClient(c, count=B_full, pack_seed=17)
    server = QueryServer(client.eval_keys(), cq, c.P0)
    eng = server.engine
    _, docs = Q.make_corpus(D, B_full, seed=21)
    qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
    docs8_small, docs8_full = server.pack_docs(docs[:B]), server.pack_docs(docs)
    payloads = client.encrypt_queries(qs)
    eng.profile(True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        return sec, out, eng.profile_read("linear_query"), eng.profile_read("blind_rotate")

    runs = {"a": lambda: server.search_many(payloads, docs8_small, B, 0.5),
            "b": lambda: [server.search(p, docs8_small, B, 0.5) for p in payloads],
            "c": lambda: server.search(payloads[0], docs8_full, B_full, 0.5)}
    orders = ("abc", "cba", "bca", "acb", "cab", "bac")
    t = {k: [] for k in runs}
    lq = {k: [] for k in runs}
    br = {k: [] for k in runs}
    last = {}
    for i in range(warmup + steps):
        for k in orders[i % len(orders)]:
            sec, out, r_lq, r_br = timed(runs[k])
            last[k] = (out, r_lq, r_br)
            if i >= warmup:
                t[k].append(sec)
                lq[k].append(r_lq["total_ms"])
                br[k].append(r_br["total_ms"])
    eng.profile(False)
    assert last["a"][1]["launches"] == 1 and last["b"][1]["launches"] == Qn and last["c"][1]["launches"] == 1
    acc_a, below_a = client.decrypt_replies(last["a"][0])
    singles = [client.decrypt_reply(r) for r in last["b"][0]]
    parity = bool(all(torch.equal(acc_a[q], s[0]) and torch.equal(below_a[q], s[1]) for q, s in enumerate(singles)))
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs[:B]) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    exact = bool(np.array_equal(acc_a.cpu().numpy(), ref) and
                 np.array_equal(below_a.cpu().numpy(), (scores < 0.5).astype(np.int64)))
    med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
    out = {"Q": Qn, "B": B, "B_full": B_full,
           "a_search_many_ms": med["a"], "a_min_ms": min(t["a"]) * 1e3,
           "b_sequential_searches_ms": med["b"], "b_min_ms": min(t["b"]) * 1e3, "b_per_search_ms": med["b"] / Qn,
           "c_full_search_ms": med["c"], "c_min_ms": min(t["c"]) * 1e3,
           "ratio_a_over_c": med["a"] / med["c"], "meets_bar_a_over_c": med["a"] <= 1.10 * med["c"],
           "ratio_a_over_b": med["a"] / med["b"], "meets_bar_a_over_b": med["a"] <= 0.5 * med["b"],
           "small_search_over_full_search": med["b"] / Qn / med["c"],
           "linear_query_ms": {k: statistics.median(v) for k, v in lq.items()},
           "linear_query_kernel_last": eng.kernel_name("linear_query"),
           "blind_rotate_ms": {k: statistics.median(v) for k, v in br.items()},
           "blind_rotate_launches": {k: last[k][2]["launches"] for k in runs},
           "reply_bytes": {"a": int(sum(r.nbytes for r in last["a"][0])),
                           "b": int(sum(r.nbytes for r in last["b"][0])), "c": int(last["c"][0].nbytes)},
           "parity_with_sequential": parity, "bit_exact": exact, "steps": steps, "warmup": warmup}
    out["meets_bar"] = out["meets_bar_a_over_c"] and out["meets_bar_a_over_b"]
    server.engine.close()
    c.engine.close()
    return out


def tenants(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Tn: int = 8, B: int = 128) -> dict:
    """Several key holders behind one host, two-party, one
    process, three things interleaved in rotating order: (a) QueryHub.search_many
    for Tn tenants x (Q = 1, B documents), each with its own keys, (b) the Tn
    QueryServer.search calls one after another, (c) one tenant's search at
    Tn * B documents. Host clock around each (reply copies included); per run
    the HIP-event split into rotations, key switches, leveled step and packings
    (the profile buckets, summed over the tenants' contexts); parity of (a)'s
    decrypted replies with (b)'s and the restatement."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.query import QueryClient, QueryHub
    from fheicp import _lib
    B_full = Tn * B
    hub, clients, corpora = QueryHub(0), [], []
    names = [f"tenant{t}" for t in range(Tn)]
    _, docs = Q.make_corpus(D, B_full, seed=21)
    qs = [Q.make_corpus(D, 1, seed=100 + t)[0] for t in range(Tn)]
    for t, name in enumerate(names):
        c = EncryptedCorpus(cq).compile(key_seed=5 + t, device=0, noise_seed=6 + t)
        client = QueryClient(c, count=B_full, pack_seed=17 + t)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0)
        hub.load(name, docs[t * B:(t + 1) * B])                      # every tenant its own documents
        clients.append(client)
        corpora.append(c)
    servers = [hub.tenants[n]["server"] for n in names]
    docs8 = [hub.tenants[n]["docs8"] for n in names]
    docs8_full = servers[0].pack_docs(docs)
    payloads = [clients[t].encrypt_queries(qs[t][None, :]) for t in range(Tn)]
    engines = [s.engine for s in servers]
    for e in engines:
        e.profile(True)
    buckets = ("blind_rotate", "keyswitch", "linear_query", "pack")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        split = {k: {"ms": 0.0, "launches": 0} for k in buckets}
        for e in engines:
            for k in buckets:
                r = e.profile_read(k)
                split[k]["ms"] += r["total_ms"]
                split[k]["launches"] += r["launches"]
        return sec, out, split

    runs = {"a": lambda: hub.search_many({n: (payloads[t], 0.5) for t, n in enumerate(names)}),
            "b": lambda: [servers[t].search(payloads[t][0], docs8[t], B, 0.5) for t in range(Tn)],
            "c": lambda: servers[0].search(payloads[0][0], docs8_full, B_full, 0.5)}
    orders = ("abc", "cba", "bca", "acb", "cab", "bac")
    t_ = {k: [] for k in runs}
    sp = {k: {b: [] for b in buckets} for k in runs}
    last = {}
    for i in range(warmup + steps):
        for k in orders[i % len(orders)]:
            sec, out, split = timed(runs[k])
            last[k] = (out, split)
            if i >= warmup:
                t_[k].append(sec)
                for b in buckets:
                    sp[k][b].append(split[b]["ms"])
    for e in engines:
        e.profile(False)
    parity = exact = True
    for t, name in enumerate(names):
        acc_a, below_a = clients[t].decrypt_replies(last["a"][0][name])
        acc_b, below_b = clients[t].decrypt_reply(last["b"][0][t])
        parity = parity and bool(torch.equal(acc_a[0], acc_b) and torch.equal(below_a[0], below_b))
        ref = Q.corpus_accumulate(oq, cq.s_e, n_bits, qs[t], docs[t * B:(t + 1) * B])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        exact = exact and bool(np.array_equal(acc_a[0].cpu().numpy(), ref) and
                               np.array_equal(below_a[0].cpu().numpy(), (scores < 0.5).astype(np.int64)))
    med = {k: statistics.median(v) * 1e3 for k, v in t_.items()}
    out = {"tenants": Tn, "Q": 1, "B": B, "B_full": B_full,
           "a_hub_search_many_ms": med["a"], "a_min_ms": min(t_["a"]) * 1e3,
           "b_sequential_searches_ms": med["b"], "b_min_ms": min(t_["b"]) * 1e3, "b_per_search_ms": med["b"] / Tn,
           "c_one_tenant_full_search_ms": med["c"], "c_min_ms": min(t_["c"]) * 1e3,
           "ratio_a_over_b": med["a"] / med["b"], "meets_bar_a_over_b": med["a"] <= 0.5 * med["b"],
           "ratio_a_over_c": med["a"] / med["c"],
           "event_split_ms": {k: {b: statistics.median(v) for b, v in sp[k].items()} for k in runs},
           "event_split_launches": {k: {b: last[k][1][b]["launches"] for b in buckets} for k in runs},
           "rotation_kernel_last_group": None,
           "parity_with_sequential": parity, "bit_exact": exact, "steps": steps, "warmup": warmup,
           "build": _lib.lib().fhe_build_info().decode()}
    # the buckets name what ran last, a single-tenant search: one more hub call names the group kernel
    hub.search_many({n: (payloads[t], 0.5) for t, n in enumerate(names)})
    out["rotation_kernel_last_group"] = engines[0].kernel_name("blind_rotate_fast")
    out["meets_bar"] = out["meets_bar_a_over_b"] and parity and exact
    for e in engines:
        e.close()
    for c in corpora:
        c.engine.close()
    return out


def private_tenants(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Tn: int = 8, B: int = 128) -> dict:
    """Several key holders' both-private searches behind one host (DESIGN.md
    §8.14), two-party, one process, three things interleaved in rotating order:
    (a) PrivateHub.search_many for Tn tenants x (Q = 1, B encrypted documents),
    each with its own keys, (b) the Tn PrivateServer.search calls one after
    another (the code path without the hub), (c) one tenant's search at Tn * B
    documents. Host clock around each (reply copies included); per run the
    HIP-event split (the profile buckets, summed over the tenants' contexts);
    parity of (a)'s decrypted replies with (b)'s and the restatement. Then the
    leveled step alone: the grouped launch sequence against the tenants' own
    fhe_linear_ggsws_batch calls on the same operands, outputs compared, at
    (Tn, B) and at (2, Tn * B / 2)."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.engine import group_rows
    from fheicp.private import PrivateClient, PrivateHub, unpack_doc_block, unpack_ggsw_query
    from fheicp import _lib
    B_full = Tn * B
    hub, clients, corpora = PrivateHub(0), [], []
    names = [f"tenant{t}" for t in range(Tn)]
    _, docs = Q.make_corpus(D, B_full, seed=21)
    qs = [Q.make_corpus(D, 1, seed=100 + t)[0] for t in range(Tn)]
    blocks = []
    for t, name in enumerate(names):
        c = EncryptedCorpus(cq).compile(key_seed=5 + t, device=0, noise_seed=6 + t)
        client = PrivateClient(c, count=B_full, pack_seed=17 + t, enc_seed=12 + t)
        hub.add_tenant(name, client.eval_keys(), cq, c.P0, scheme=c.scheme)
        blocks.append(client.encrypt_docs(docs[t * B:(t + 1) * B]))      # every tenant its own documents
        hub.load(name, blocks[t])
        clients.append(client)
        corpora.append(c)
    servers = [hub.tenants[n]["server"] for n in names]
    gadget = (servers[0].base_log, servers[0].level)
    docs8 = [servers[t].pack_docs(blocks[t])[0] for t in range(Tn)]
    docs8_full = servers[0].pack_docs(clients[0].encrypt_docs(docs))[0]
    payloads = [clients[t].encrypt_queries(qs[t][None, :]) for t in range(Tn)]
    engines = [s.engine for s in servers]
    for e in engines:
        e.profile(True)
    buckets = ("blind_rotate", "keyswitch", "linear_ggsws", "linear_ggsw", "pack")

    def read_split():
        split = {k: {"ms": 0.0, "launches": 0} for k in buckets}
        for e in engines:
            for k in buckets:
                r = e.profile_read(k)
                split[k]["ms"] += r["total_ms"]
                split[k]["launches"] += r["launches"]
        return split

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, read_split()

    runs = {"a": lambda: hub.search_many({n: (payloads[t], 0.5) for t, n in enumerate(names)}),
            "b": lambda: [servers[t].search(payloads[t][0], docs8[t], B, 0.5) for t in range(Tn)],
            "c": lambda: servers[0].search(payloads[0][0], docs8_full, B_full, 0.5)}
    orders = ("abc", "cba", "bca", "acb", "cab", "bac")
    t_ = {k: [] for k in runs}
    sp = {k: {b: [] for b in buckets} for k in runs}
    last = {}
    for i in range(warmup + steps):
        for k in orders[i % len(orders)]:
            sec, out, split = timed(runs[k])
            last[k] = (out, split)
            if i >= warmup:
                t_[k].append(sec)
                for b in buckets:
                    sp[k][b].append(split[b]["ms"])
    parity = exact = True
    for t, name in enumerate(names):
        acc_a, below_a = clients[t].decrypt_replies(last["a"][0][name])
        acc_b, below_b = clients[t].decrypt_reply(last["b"][0][t])
        parity = parity and bool(torch.equal(acc_a[0], acc_b) and torch.equal(below_a[0], below_b))
        ref = Q.corpus_accumulate(oq, cq.s_e, n_bits, qs[t], docs[t * B:(t + 1) * B])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        exact = exact and bool(np.array_equal(acc_a[0].cpu().numpy(), ref) and
                               np.array_equal(below_a[0].cpu().numpy(), (scores < 0.5).astype(np.int64)))
    med = {k: statistics.median(v) * 1e3 for k, v in t_.items()}
    out = {"tenants": Tn, "Q": 1, "B": B, "B_full": B_full, "gadget": list(gadget),
           "a_hub_search_many_ms": med["a"], "a_min_ms": min(t_["a"]) * 1e3,
           "b_sequential_searches_ms": med["b"], "b_min_ms": min(t_["b"]) * 1e3, "b_per_search_ms": med["b"] / Tn,
           "c_one_tenant_full_search_ms": med["c"], "c_min_ms": min(t_["c"]) * 1e3,
           "ratio_a_over_b": med["a"] / med["b"], "meets_bar_a_over_b": med["a"] <= 0.5 * med["b"],
           "ratio_a_over_c": med["a"] / med["c"],
           "event_split_ms": {k: {b: statistics.median(v) for b, v in sp[k].items()} for k in runs},
           "event_split_launches": {k: {b: last[k][1][b]["launches"] for b in buckets} for k in runs},
           "parity_with_sequential": parity, "bit_exact": exact, "steps": steps, "warmup": warmup,
           "build": _lib.lib().fhe_build_info().decode()}

    # the leveled step alone: one grouped launch sequence against the tenants' own calls
    def leveled(Tl, Bl):
        grp = hub.group()
        items = [None] * Tn
        for t in range(Tl):
            eng = engines[t]
            bl = unpack_doc_block(clients[t].encrypt_docs(docs[t * Bl:(t + 1) * Bl]))
            dq = eng.pack_docs_glwe_queries(eng.to_dev(bl["glwe"]), Bl, D, *gadget)
            g = eng.to_dev(unpack_ggsw_query(payloads[t][0])["ggsw"])
            items[t] = (g, gadget[0], gadget[1], dq, Bl, D)
        csts = [None if it is None else [3 + t] for t, it in enumerate(items)]
        M, starts = group_rows([Bl if it is not None else 0 for it in items])
        buf = torch.empty((M, engines[0].W), dtype=torch.int64, device=engines[0].device)
        own = [torch.empty((Bl, engines[0].W), dtype=torch.int64, device=engines[0].device) for _ in range(Tl)]
        legs = {"grouped": lambda: grp.linear_ggsws(items, csts, out=buf),
                "per_tenant": lambda: [engines[t].linear_ggsws(*items[t], csts[t], out=own[t]) for t in range(Tl)]}
        ms = {k: [] for k in legs}
        nl = {}
        read_split()
        for i in range(warmup + steps):
            for k in (("grouped", "per_tenant") if i % 2 == 0 else ("per_tenant", "grouped")):
                legs[k]()
                torch.cuda.synchronize()
                r = read_split()["linear_ggsws"]
                nl[k] = r["launches"]
                if i >= warmup:
                    ms[k].append(r["ms"])
        same = all(torch.equal(buf[starts[t]:starts[t] + Bl], own[t]) for t in range(Tl))
        g_ms, p_ms = statistics.median(ms["grouped"]), statistics.median(ms["per_tenant"])
        return {"T": Tl, "B": Bl, "grouped_ms": g_ms, "per_tenant_sum_ms": p_ms, "ratio": g_ms / p_ms,
                "grouped_brackets": nl["grouped"], "per_tenant_brackets": nl["per_tenant"],
                "identical_words": bool(same), "meets_bar": bool(g_ms < p_ms and same)}
    out["leveled"] = [leveled(Tn, B), leveled(2, B_full // 2)]
    for e in engines:
        e.profile(False)
    # the buckets name what ran last: one more hub call names the group kernels
    hub.search_many({n: (payloads[t], 0.5) for t, n in enumerate(names)})
    out["leveled_kernel_group"] = engines[0].kernel_name("linear_ggsws")
    out["rotation_kernel_last_group"] = engines[0].kernel_name("blind_rotate_fast")
    out["meets_bar"] = bool(out["meets_bar_a_over_b"] and parity and exact and all(l["meets_bar"] for l in out["leveled"]))
    hub.close()
    for e in engines:
        e.close()
    for c in corpora:
        c.engine.close()
    return out


def stored_tenants(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Tn: int = 8, B: int = 128) -> dict:
    """Several key holders' STORED documents behind one host,
    two-party, one process. Two passes, none and all of every tenant's
    documents old-generation (rotated tenants, bridged rows); per pass three
    legs interleaved in rotating order: (a) CorpusHub.search_many for Tn
    tenants x (Q = 1, B documents), (b) the Tn CorpusServer.search calls one
    after another, (c) one tenant's search at Tn * B documents. Host clock
    around each (reply copies included); per run the HIP-event split into
    rotations, key switches, bridge, packings and leveled step (the profile
    buckets, summed over the tenants' contexts); parity of (a)'s decrypted
    replies with (b)'s and the restatement."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusHub, CorpusServer
    from fheicp import _lib
    B_full = Tn * B
    names = [f"tenant{t}" for t in range(Tn)]
    _, docs = Q.make_corpus(D, B_full, seed=21)
    qs = [Q.make_corpus(D, 1, seed=100 + t)[0] for t in range(Tn)]
    buckets = ("blind_rotate", "keyswitch", "bridge", "pack", "linear_seeded")
    orders = ("abc", "cba", "bca", "acb", "cab", "bac")
    out = {"tenants": Tn, "Q": 1, "B": B, "B_full": B_full, "steps": steps, "warmup": warmup,
           "build": _lib.lib().fhe_build_info().decode(), "passes": {}}
    for pass_name in ("none_old", "all_old"):
        hub, clients, corpora = CorpusHub(0), [], []
        for t, name in enumerate(names):
            c = EncryptedCorpus(cq).compile(key_seed=5 + t, device=0, noise_seed=6 + t)
            client = CorpusClient(c, count=1024, pack_seed=17 + t)
            corpora.append(c)
            mine = docs[t * B:(t + 1) * B]                               # every tenant its own documents
            hub.add_tenant(name, client.eval_keys(), cq, c.P0, c.mask_key)
            hub.load(name, *client.encrypt_docs(mine))
            if pass_name == "all_old":
                client = client.rotate(key_seed=50 + t, pack_seed=60 + t, bridge_seed=70 + t, noise_seed=80 + t)
                corpora.append(client.corpus)
                hub.rekey(name, client.eval_keys())
            clients.append(client)
        servers = [hub.tenants[n] for n in names]
        # leg (c): tenant 0's generation holds all Tn * B documents (old-generation in the rotated pass)
        full = CorpusServer(clients[0].eval_keys(), cq, corpora[0].P0, corpora[0].mask_key)
        if pass_name == "all_old":
            first = CorpusClient.__new__(CorpusClient)
            first.__dict__.update(clients[0].__dict__)
            first.corpus = corpora[0]
            full.load(*first.encrypt_docs(docs))
            full.b_old, full.old_key_id = B_full, clients[0].bridge_from
        else:
            full.load(*clients[0].encrypt_docs(docs))
        engines = [s.engine for s in servers] + [full.engine]
        for e in engines:
            e.profile(True)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            split = {k: {"ms": 0.0, "launches": 0} for k in buckets}
            for e in engines:
                for k in buckets:
                    r = e.profile_read(k)
                    split[k]["ms"] += r["total_ms"]
                    split[k]["launches"] += r["launches"]
            return sec, res, split

        runs = {"a": lambda: hub.search_many({n: (qs[t][None, :], 0.5) for t, n in enumerate(names)}),
                "b": lambda: [servers[t].search(qs[t], 0.5) for t in range(Tn)],
                "c": lambda: full.search(qs[0], 0.5)}
        t_ = {k: [] for k in runs}
        sp = {k: {b: [] for b in buckets} for k in runs}
        last = {}
        for i in range(warmup + steps):
            for k in orders[i % len(orders)]:
                sec, res, split = timed(runs[k])
                last[k] = (res, split)
                if i >= warmup:
                    t_[k].append(sec)
                    for b in buckets:
                        sp[k][b].append(split[b]["ms"])
        for e in engines:
            e.profile(False)
        parity = exact = True
        for t, name in enumerate(names):
            acc_a, below_a = clients[t].decrypt_replies(last["a"][0][name])
            acc_b, below_b = clients[t].decrypt_replies(last["b"][0][t])
            parity = parity and bool(torch.equal(acc_a, acc_b) and torch.equal(below_a, below_b))
            ref = Q.corpus_accumulate(oq, cq.s_e, n_bits, qs[t], docs[t * B:(t + 1) * B])
            scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
            exact = exact and bool(np.array_equal(acc_a[0].cpu().numpy(), ref) and
                                   np.array_equal(below_a[0].cpu().numpy(), (scores < 0.5).astype(np.int64)))
        med = {k: statistics.median(v) * 1e3 for k, v in t_.items()}
        hub.search_many({n: (qs[t][None, :], 0.5) for t, n in enumerate(names)})  # names what the hub launched
        res = {"a_hub_search_many_ms": med["a"], "a_min_ms": min(t_["a"]) * 1e3,
               "b_sequential_searches_ms": med["b"], "b_min_ms": min(t_["b"]) * 1e3, "b_per_search_ms": med["b"] / Tn,
               "c_one_tenant_full_search_ms": med["c"], "c_min_ms": min(t_["c"]) * 1e3,
               "ratio_a_over_b": med["a"] / med["b"], "meets_bar_a_over_b": med["a"] <= 0.5 * med["b"],
               "ratio_a_over_c": med["a"] / med["c"],
               "event_split_ms": {k: {b: statistics.median(v) for b, v in sp[k].items()} for k in runs},
               "event_split_launches": {k: {b: last[k][1][b]["launches"] for b in buckets} for k in runs},
               "keyswitch_kernel_last_group": engines[0].kernel_name("keyswitch"),
               "rounds": [r["mode"] for r in hub.rounds({n: (qs[t][None, :], 0.5) for t, n in enumerate(names)})],
               "parity_with_sequential": parity, "bit_exact": exact}
        res["meets_bar"] = res["meets_bar_a_over_b"] and parity and exact
        out["passes"][pass_name] = res
        for e in engines:
            e.close()
        for c in corpora:
            c.engine.close()
    out["meets_bar"] = all(p["meets_bar"] for p in out["passes"].values())
    return out


def stored_tenants_gens(cq, oq, D: int, n_bits: int, G: int, steps: int, warmup: int, Tn: int = 8, B: int = 128,
                        Qn: int = 8, plain_first: bool = False) -> dict:
    """Rotation schedules in the stored-ciphertext hub, one
    process: Tn tenants x (Qn queries, B documents), every tenant's documents
    in G old generations in equal parts and none current (as --rotated
    --generations splits them). Leg "sched": CorpusHub(rotation_schedules=True),
    one grouped bridge pass over all tenants' generations. At G = 1 also leg
    "plain": the default hub, one single-key bridge per tenant; the two hubs
    alternate, their order swapping every step. Host clock around each
    search_many with a device synchronise; per run the "bridge" bucket summed
    over the hub's contexts; each leg's decrypted replies against the
    restatement, and at G = 1 the two hubs' replies word for word."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusHub
    from fheicp import _lib
    names = [f"tenant{t}" for t in range(Tn)]
    _, docs = Q.make_corpus(D, Tn * B, seed=21)
    qs = [np.stack([Q.make_corpus(D, 1, seed=100 + Qn * t + i)[0] for i in range(Qn)]) for t in range(Tn)]
    ends = [B * (g + 1) // G for g in range(G)]
    lo = [0] + ends[:-1]
    hubs = {"sched": CorpusHub(0, rotation_schedules=True)}
    if G == 1:
        hubs["plain"] = CorpusHub(0)
    if plain_first:  # the default hub's servers are built, and run, before the other's
        hubs = dict(reversed(list(hubs.items())))
    news, engines = [], []
    for t, name in enumerate(names):
        c0 = EncryptedCorpus(cq).compile(key_seed=5 + 16 * t, device=0, noise_seed=6 + 16 * t)
        clients = [CorpusClient(c0, count=1024, pack_seed=17 + 16 * t)]
        for g in range(1, G):
            clients.append(clients[-1].rotate(key_seed=5 + 16 * t + 2 * g, pack_seed=17 + 16 * t + g,
                                              bridge_seed=1000 + 16 * t + g, noise_seed=6 + 16 * t + 2 * g))
        new = clients[-1].rotate(key_seed=5 + 16 * t + 2 * G, pack_seed=17 + 16 * t + G, bridge_seed=2000 + 16 * t,
                                 noise_seed=6 + 16 * t + 2 * G, bridge_from=clients)
        mine = docs[t * B:(t + 1) * B]
        enc = [c.encrypt_docs(mine[lo[g]:ends[g]]) for g, c in enumerate(clients)]
        keys = new.eval_keys()                                          # bridge g in slot g
        for hub in hubs.values():
            s = hub.add_tenant(name, keys, cq, c0.P0, c0.mask_key)
            s.load(np.concatenate([e[0] for e in enc]), np.concatenate([e[1] for e in enc]))
            s.b_old, s.old_key_id = B, clients[0].key_id
            if G > 1:
                s._old_gens, s._gen_slots = [(c.key_id, ends[g]) for g, c in enumerate(clients)], list(range(G))
            engines.append(s.engine)
        news.append(new)
        for c in clients:
            c.corpus.engine.close()
    requests = {n: (qs[t], 0.5) for t, n in enumerate(names)}
    for e in engines:
        e.profile(True)

    def timed(hub):
        for s in hub.tenants.values():
            s.engine.profile_read("bridge")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = hub.search_many(requests)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        br = [s.engine.profile_read("bridge") for s in hub.tenants.values()]
        return sec, res, sum(r["total_ms"] for r in br), sum(r["launches"] for r in br)

    legs = list(hubs)
    t_, br_, last, brackets = {k: [] for k in legs}, {k: [] for k in legs}, {}, {}
    for i in range(warmup + steps):
        for k in (legs if i % 2 == 0 else legs[::-1]):
            sec, last[k], ms, brackets[k] = timed(hubs[k])
            if i >= warmup:
                t_[k].append(sec)
                br_[k].append(ms)
    for e in engines:
        e.profile(False)
    exact = {}
    for k in legs:
        ok = True
        for t, name in enumerate(names):
            acc, below = news[t].decrypt_replies(last[k][name])
            ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs[t * B:(t + 1) * B]) for q in qs[t]])
            scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
            ok = ok and bool(np.array_equal(acc.cpu().numpy(), ref) and
                             np.array_equal(below.cpu().numpy(), (scores < 0.5).astype(np.int64)))
        exact[k] = ok
    out = {"tenants": Tn, "Q": Qn, "B": B, "generations": G, "steps": steps, "warmup": warmup,
           "build": _lib.lib().fhe_build_info().decode(), "bridge_gadget": list(news[0].bridge_gadget),
           "hub_order": list(hubs), "rounds": [r["mode"] for r in hubs["sched"].rounds(requests)],
           "rows_bridged": Tn * Qn * B, "blocks": Tn * sum(-(-Qn * (e - l) // 128) for l, e in zip(lo, ends)),
           "bridge_kernel_sched": next(iter(hubs["sched"].tenants.values())).engine.kernel_name("bridge"),
           "legs": {k: {"search_ms": statistics.median(t_[k]) * 1e3, "search_min_ms": min(t_[k]) * 1e3,
                        "bridge_ms_per_search": statistics.median(br_[k]), "bridge_min_ms": min(br_[k]),
                        "bridge_brackets_per_search": brackets[k], "bit_exact": exact[k]} for k in legs}}
    if G == 1:
        out["replies_equal_word_for_word"] = all(
            len(last["sched"][n]) == len(last["plain"][n]) and
            all(np.array_equal(a, b) for a, b in zip(last["sched"][n], last["plain"][n])) for n in names)
        out["ratio_sched_over_plain_search"] = out["legs"]["sched"]["search_ms"] / out["legs"]["plain"]["search_ms"]
        out["ratio_sched_over_plain_bridge"] = (out["legs"]["sched"]["bridge_ms_per_search"] /
                                                out["legs"]["plain"]["bridge_ms_per_search"])
    out["bit_exact"] = all(exact.values()) and out.get("replies_equal_word_for_word", True)
    for hub in hubs.values():
        hub.close()
    for n in news:
        n.corpus.engine.close()
    return out


def stored_leveled(eng, D: int, steps: int, warmup: int, Qn: int = 8, sizes=(128, 1024)) -> dict:
    """The stored-ciphertext leveled step for Qn queries, per document count:
    one fhe_linear_seeded_queries_batch (the "linear_seeded" bucket, and HIP
    events around the call) against Qn fhe_linear_seeded_batch calls on the
    same documents (HIP events around the Qn calls), interleaved in
    alternating order; the outputs compared word for word. Needs no keys."""
    import numpy as np
    import torch
    rng = np.random.default_rng(5)
    mk = np.arange(8, dtype=np.uint32) + 5
    out = {}
    eng.profile(True)
    for B in sizes:
        body = eng.to_dev(rng.integers(0, 2 ** 63, (B, D), dtype=np.int64))
        ids = eng.to_dev(rng.integers(0, 2 ** 63, B, dtype=np.int64))
        W = rng.integers(-(2 ** 20), 2 ** 20, (Qn, D), dtype=np.int64)
        Wd, rows = eng.to_dev(W), [eng.to_dev(W[q]) for q in range(Qn)]
        cst = list(range(Qn))
        buf = eng.empty_big(Qn * B)

        def ev(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), r

        runs = {"batched": lambda: eng.linear_seeded_queries(body, ids, mk, Wd, cst, out=buf),
                "sequential": lambda: [eng.linear_seeded(body, ids, mk, rows[q], cst[q]) for q in range(Qn)]}
        t = {k: [] for k in runs}
        bucket, last = [], {}
        for i in range(warmup + steps):
            for k in (("batched", "sequential") if i % 2 else ("sequential", "batched")):
                ms, last[k] = ev(runs[k])
                if k == "batched":
                    r = eng.profile_read("linear_seeded")
                    assert r["launches"] == 1 and r["items"] == Qn * B
                if i >= warmup:
                    t[k].append(ms)
                    if k == "batched":
                        bucket.append(r["total_ms"])
        equal = bool(torch.equal(last["batched"], torch.cat(last["sequential"])))
        b_ms, s_ms = statistics.median(bucket), statistics.median(t["sequential"])
        out[f"B{B}"] = {"Q": Qn, "B": B, "D": D, "linear_seeded_bucket_ms": b_ms, "bucket_min_ms": min(bucket),
                        "batched_call_ms": statistics.median(t["batched"]), "sequential_calls_ms": s_ms,
                        "sequential_min_ms": min(t["sequential"]), "ratio_batched_over_sequential": b_ms / s_ms,
                        "meets_bar": b_ms < s_ms, "equal_words": equal}
    eng.profile(False)
    out["kernel"] = eng.kernel_name("linear_seeded")
    return out


def stored_queries(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Qn: int = 8, B: int = 128,
                   B_full: int = 1024) -> dict:
    """The stored-ciphertext search for several queries, one
    process, three things interleaved in rotating order as multi_query does:
    (a) CorpusServer.search_many with Qn queries against B resident
    documents, (b) Qn sequential CorpusServer.search calls against the same
    documents, (c) one EncryptedCorpus.compare against B_full = Qn * B
    documents on the key holder's context (the same ciphertext count as (a)).
    Host clock around each with a device synchronise (reply copies included),
    and the parity of (a)'s decrypted replies with (b)'s and the restatement."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusServer
    assert Qn * B == B_full
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    client = CorpusClient(c, count=B_full, pack_seed=17)
    server = CorpusServer(client.eval_keys(), cq, c.P0, c.mask_key)
    _, docs = Q.make_corpus(D, B_full, seed=21)
    qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
    bodies, ids = client.encrypt_docs(docs)
    server.load(bodies[:B], ids[:B])
    bd_full, id_full = c.engine.to_dev(bodies), c.engine.to_dev(ids)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    runs = {"a": lambda: server.search_many(qs, 0.5),
            "b": lambda: [server.search(q, 0.5) for q in qs],
            "c": lambda: c.compare(bd_full, id_full, qs[0], 0.5)}
    orders = ("abc", "cba", "bca", "acb", "cab", "bac")
    t = {k: [] for k in runs}
    last = {}
    for i in range(warmup + steps):
        for k in orders[i % len(orders)]:
            sec, last[k] = timed(runs[k])
            if i >= warmup:
                t[k].append(sec)
    acc_a, below_a = client.decrypt_replies(last["a"])
    singles = [client.decrypt_replies(r) for r in last["b"]]
    parity = bool(all(torch.equal(acc_a[q], s[0][0]) and torch.equal(below_a[q], s[1][0])
                      for q, s in enumerate(singles)))
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs[:B]) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    exact = bool(np.array_equal(acc_a.cpu().numpy(), ref) and
                 np.array_equal(below_a.cpu().numpy(), (scores < 0.5).astype(np.int64)))
    ref_c = Q.corpus_accumulate(oq, cq.s_e, n_bits, qs[0], docs)
    exact_c = bool(np.array_equal(last["c"][0].cpu().numpy(), ref_c))
    med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
    out = {"Q": Qn, "B": B, "B_full": B_full, "pack_gadget": [client.base_log, client.level],
           "pack_margin_sigmas": client.margin, "in_var": client.in_var,
           "a_search_many_ms": med["a"], "a_min_ms": min(t["a"]) * 1e3,
           "b_sequential_searches_ms": med["b"], "b_min_ms": min(t["b"]) * 1e3, "b_per_search_ms": med["b"] / Qn,
           "c_full_compare_ms": med["c"], "c_min_ms": min(t["c"]) * 1e3,
           "ratio_a_over_b": med["a"] / med["b"], "meets_bar_a_over_b": med["a"] <= 0.5 * med["b"],
           "ratio_a_over_c": med["a"] / med["c"], "meets_bar_a_over_c": med["a"] <= 1.10 * med["c"],
           "reply_bytes": {"a": int(sum(r.nbytes for r in last["a"])), "b": int(sum(r.nbytes for r in last["b"]))},
           "parity_with_sequential": parity, "bit_exact": exact, "full_compare_bit_exact": exact_c,
           "steps": steps, "warmup": warmup}
    out["leveled"] = stored_leveled(server.engine, D, steps, warmup, Qn, (B, B_full))
    out["meets_bar"] = bool(out["meets_bar_a_over_b"] and out["meets_bar_a_over_c"] and
                            all(v["meets_bar"] for k, v in out["leveled"].items() if k != "kernel"))
    server.engine.close()
    c.engine.close()
    return out


def rotated(cq, oq, D: int, n_bits: int, steps: int, warmup: int, shapes=((8, 128), (1, 1024))) -> dict:
    """The stored-ciphertext search after a key rotation, one
    process, one evaluation-only server holding the NEW generation's keys and
    its bridge key. Per shape (Q queries x B documents) three legs, interleaved
    in rotating order as stored_queries does: every document old-generation
    (B_old = B), half of them (B_old = B / 2), none (B_old = 0, the unbridged
    entry). Host clock around each search_many with a device synchronise (reply
    copies included); then a short profiled pass for the "bridge" and "pack"
    HIP-event buckets; and the parity of every leg's decrypted replies with
    the restatement."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusServer
    Bmax = max(B for _, B in shapes)
    c0 = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    client0 = CorpusClient(c0, count=1024, pack_seed=17)
    client1 = client0.rotate(key_seed=7, pack_seed=18, bridge_seed=19, noise_seed=20)
    server = CorpusServer(client1.eval_keys(), cq, c0.P0, c0.mask_key)
    eng = server.engine
    _, docs = Q.make_corpus(D, Bmax, seed=21)
    old_b, old_i = client0.encrypt_docs(docs)
    new_b, new_i = client1.encrypt_docs(docs)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    out = {"bridge_gadget": list(client1.bridge_gadget), "pack_gadget": [client1.base_log, client1.level],
           "pack_gadget_unrotated": [client0.base_log, client0.level], "pack_margin_sigmas": client1.margin,
           "bridge_key_bytes": 8 * eng.bridge_key_words(*client1.bridge_gadget), "steps": steps, "warmup": warmup,
           "shapes": []}
    for Qn, B in shapes:
        qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
        legs = {}
        for name, n_old in (("all_old", B), ("half_old", B // 2), ("none_old", 0)):
            body = np.concatenate([old_b[:n_old], new_b[n_old:B]])
            ids = np.concatenate([old_i[:n_old], new_i[n_old:B]])
            legs[name] = (eng.to_dev(body), eng.to_dev(ids), n_old)

        def run(name):
            server.body, server.ids, server.b_old = legs[name]
            return server.search_many(qs, 0.5)

        orders = ("abc", "cba", "bca", "acb", "cab", "bac")
        names = {"a": "all_old", "b": "half_old", "c": "none_old"}
        t = {k: [] for k in legs}
        last = {}
        for i in range(warmup + steps):
            for k in orders[i % len(orders)]:
                sec, last[names[k]] = timed(lambda: run(names[k]))
                if i >= warmup:
                    t[names[k]].append(sec)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs[:B]) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        exact = {}
        for name in legs:
            acc, below = client1.decrypt_replies(last[name])
            exact[name] = bool(np.array_equal(acc.cpu().numpy(), ref) and
                               np.array_equal(below.cpu().numpy(), (scores < 0.5).astype(np.int64)))
        # the HIP-event split, in a pass of its own (the brackets are not in the timed runs)
        eng.profile(True)
        split = {}
        for name in legs:
            for kern in ("bridge", "pack", "linear_seeded"):
                eng.profile_read(kern)
            for _ in range(5):
                run(name)
            torch.cuda.synchronize()
            split[name] = {kern: eng.profile_read(kern)["total_ms"] / 5 for kern in ("bridge", "pack", "linear_seeded")}
        eng.profile(False)
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        out["shapes"].append({
            "Q": Qn, "B": B, "ms_per_search": med, "min_ms": {k: min(v) * 1e3 for k, v in t.items()},
            "ratio_over_none_old": {k: med[k] / med["none_old"] for k in med},
            "event_ms_per_search": split, "bridge_kernel": eng.kernel_name("bridge"), "bit_exact": exact})
    out["bit_exact"] = all(all(s["bit_exact"].values()) for s in out["shapes"])
    eng.close()
    c0.engine.close()
    client1.corpus.engine.close()
    return out


def rotated_gens(cq, oq, D: int, n_bits: int, G: int, steps: int, warmup: int, shapes=((8, 128), (1, 1024))) -> dict:
    """The stored-ciphertext search with G old generations resident (DESIGN.md
    §8.17), one process, one evaluation-only server holding the newest
    generation's keys and a direct bridge key from each of the G old ones. Per
    shape three legs, interleaved in rotating order as rotated() does: the G
    old generations in equal parts of the B documents (the generation row map:
    fhe_search_seeded_queries_gens_batch), all B documents of ONE old
    generation (the single bridge of §8.12 over the same row count), none old.
    Host clock around each search_many with a device synchronise; then a short
    profiled pass for the "bridge", "pack" and "linear_seeded" HIP-event
    buckets; and the parity of every leg's decrypted replies with the
    restatement."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.stored import CorpusClient, CorpusServer
    Bmax = max(B for _, B in shapes)
    c0 = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    clients = [CorpusClient(c0, count=1024, pack_seed=17)]
    for g in range(1, G):
        clients.append(clients[-1].rotate(key_seed=5 + 2 * g, pack_seed=17 + g, bridge_seed=100 + g,
                                          noise_seed=6 + 2 * g))
    new = clients[-1].rotate(key_seed=5 + 2 * G, pack_seed=17 + G, bridge_seed=200, noise_seed=6 + 2 * G,
                             bridge_from=clients)
    server = CorpusServer(new.eval_keys(), cq, c0.P0, c0.mask_key)
    eng = server.engine
    _, docs = Q.make_corpus(D, Bmax, seed=21)
    enc = [c.encrypt_docs(docs) for c in clients]
    new_b, new_i = new.encrypt_docs(docs)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    out = {"generations": G, "bridge_gadget": list(new.bridge_gadget), "pack_gadget": [new.base_log, new.level],
           "bridge_key_bytes_each": 8 * eng.bridge_key_words(*new.bridge_gadget), "steps": steps, "warmup": warmup,
           "shapes": []}
    for Qn, B in shapes:
        qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
        ends = [B * (g + 1) // G for g in range(G)]
        lo = [0] + ends[:-1]
        legs = {
            "gens_old": (eng.to_dev(np.concatenate([enc[g][0][lo[g]:ends[g]] for g in range(G)])),
                         eng.to_dev(np.concatenate([enc[g][1][lo[g]:ends[g]] for g in range(G)])), B,
                         [(clients[g].key_id, ends[g]) for g in range(G)], list(range(G))),
            "one_old": (eng.to_dev(enc[0][0][:B]), eng.to_dev(enc[0][1][:B]), B, None, None),
            "none_old": (eng.to_dev(new_b[:B]), eng.to_dev(new_i[:B]), 0, None, None)}

        def run(name):
            server.body, server.ids, server.b_old, server._old_gens, server._gen_slots = legs[name]
            return server.search_many(qs, 0.5)

        orders = ("abc", "cba", "bca", "acb", "cab", "bac")
        names = {"a": "gens_old", "b": "one_old", "c": "none_old"}
        t = {k: [] for k in legs}
        last = {}
        for i in range(warmup + steps):
            for k in orders[i % len(orders)]:
                sec, last[names[k]] = timed(lambda: run(names[k]))
                if i >= warmup:
                    t[names[k]].append(sec)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs[:B]) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        exact = {}
        for name in legs:
            acc, below = new.decrypt_replies(last[name])
            exact[name] = bool(np.array_equal(acc.cpu().numpy(), ref) and
                               np.array_equal(below.cpu().numpy(), (scores < 0.5).astype(np.int64)))
        # the HIP-event split, in passes of their own (the brackets are not in the timed runs):
        # three rounds of five searches per leg, so the bucket has a spread of its own
        eng.profile(True)
        split, kernels = {name: [] for name in legs}, {}
        for _ in range(3):
            for name in legs:
                for kern in ("bridge", "pack", "linear_seeded"):
                    eng.profile_read(kern)
                for _ in range(5):
                    run(name)
                torch.cuda.synchronize()
                split[name].append({kern: eng.profile_read(kern)["total_ms"] / 5
                                    for kern in ("bridge", "pack", "linear_seeded")})
                kernels[name] = eng.kernel_name("bridge")
        eng.profile(False)
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        out["shapes"].append({
            "Q": Qn, "B": B, "ends": ends, "ms_per_search": med, "min_ms": {k: min(v) * 1e3 for k, v in t.items()},
            "ratio_over_none_old": {k: med[k] / med["none_old"] for k in med},
            "event_ms_per_search": {k: {kern: statistics.median(r[kern] for r in v) for kern in v[0]}
                                    for k, v in split.items()},
            "bridge_event_ms_rounds": {k: [r["bridge"] for r in v] for k, v in split.items()},
            "bridge_kernel": kernels, "bit_exact": exact})
    out["bit_exact"] = all(all(s["bit_exact"].values()) for s in out["shapes"])
    eng.close()
    for c in clients + [new]:
        c.corpus.engine.close()
    return out


def private_leveled(eng, beta: int, L: int, D: int, steps: int, warmup: int, Qn: int = 8, sizes=(128, 1024)) -> dict:
    """The both-private leveled step for Qn GGSW queries, per document count:
    one fhe_linear_ggsws_batch (the "linear_ggsws" bucket, and HIP events
    around the call) against Qn fhe_linear_ggsw_batch calls on the same
    documents (HIP events around the Qn calls, and the sum of their
    "linear_ggsw" buckets), interleaved in alternating order; the outputs
    compared word for word. Then the same at Q = 1 (reported only). Arbitrary
    words stand for the ciphertexts: the step is exact modulo 2^64 and needs
    no keys."""
    import numpy as np
    import torch
    rng = np.random.default_rng(13)
    p = eng.params
    out = {}
    eng.profile(True)
    words = eng.ggsw_words(beta, L)
    ggsws = eng.to_dev(rng.integers(0, 2 ** 64, (Qn, words), dtype=np.uint64))
    singles = [ggsws[q].contiguous() for q in range(Qn)]

    def ev(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for B in sizes:
        G = eng.doc_glwes(B, D)
        glwe = eng.to_dev(rng.integers(0, 2 ** 64, (G, (p.k + 1) * p.N), dtype=np.uint64))
        docs8, docsq = eng.pack_docs_glwe(glwe, B, D, beta, L), eng.pack_docs_glwe_queries(glwe, B, D, beta, L)
        cst = list(range(-3, Qn - 3))
        buf = eng.empty_big(Qn * B)
        for Qr in (Qn, 1):
            runs = {"batched": lambda: eng.linear_ggsws(ggsws[:Qr], beta, L, docsq, B, D, cst[:Qr], out=buf[:Qr * B]),
                    "sequential": lambda: [eng.linear_ggsw(singles[q], beta, L, docs8, B, D, cst[q])
                                           for q in range(Qr)]}
            t = {k: [] for k in runs}
            bucket, seq_bucket, last = [], [], {}
            for i in range(warmup + steps):
                for k in (("batched", "sequential") if i % 2 else ("sequential", "batched")):
                    ms, last[k] = ev(runs[k])
                    if k == "batched":
                        r = eng.profile_read("linear_ggsws")
                        assert r["launches"] == 1 and r["items"] == Qr * B
                    else:
                        rs = eng.profile_read("linear_ggsw")
                        assert rs["launches"] == Qr
                    if i >= warmup:
                        t[k].append(ms)
                        if k == "batched":
                            bucket.append(r["total_ms"])
                        else:
                            seq_bucket.append(rs["total_ms"])
            equal = bool(torch.equal(last["batched"], torch.cat(last["sequential"])))
            b_ms, s_ms = statistics.median(bucket), statistics.median(t["sequential"])
            row = {"Q": Qr, "B": B, "D": D, "doc_glwes": G, "linear_ggsws_bucket_ms": b_ms,
                   "bucket_min_ms": min(bucket), "batched_call_ms": statistics.median(t["batched"]),
                   "sequential_calls_ms": s_ms, "sequential_min_ms": min(t["sequential"]),
                   "sequential_linear_ggsw_buckets_ms": statistics.median(seq_bucket),
                   "ratio_batched_over_sequential": b_ms / s_ms, "equal_words": equal,
                   "kernel": eng.kernel_name("linear_ggsws")}
            if Qr == Qn:
                row["meets_bar"] = bool(b_ms < s_ms and equal)
            out[f"B{B}" if Qr == Qn else f"B{B}_Q1"] = row
    eng.profile(False)
    out["ws_bytes"] = eng.ggsws_ws_bytes(Qn, max(sizes), D, L)
    out["toeplitz_plane_bytes_per_query"] = ((p.k + 1) * p.N) ** 2 * L * 8
    return out


def private_queries(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Qn: int = 8, B: int = 128,
                    B_full: int = 1024) -> dict:
    """The both-private search for several GGSW queries, one
    process, three things interleaved in rotating order as multi_query does:
    (a) PrivateServer.search_many with Qn queries against B documents, (b) Qn
    sequential PrivateServer.search calls against the same documents, (c) one
    PrivateServer.search against B_full = Qn * B documents (the same
    ciphertext count as (a)). Host clock around each with a device
    synchronise (payload parse and upload, reply copies included), and the
    parity of (a)'s decrypted replies with (b)'s and the restatement."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.private import PrivateClient, PrivateServer
    assert Qn * B == B_full
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    client = PrivateClient(c, count=B_full, pack_seed=17, enc_seed=18)
    server = PrivateServer(client.eval_keys(), cq, c.P0, scheme=c.scheme)
    _, docs = Q.make_corpus(D, B_full, seed=21)
    qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
    block_small, block_full = client.encrypt_docs(docs[:B]), client.encrypt_docs(docs)
    docs8_small, _ = server.pack_docs(block_small)
    docs8_full, _ = server.pack_docs(block_full)
    docsq_small, _ = server.pack_docs_many(block_small)
    payloads = client.encrypt_queries(qs)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    runs = {"a": lambda: server.search_many(payloads, docsq_small, B, 0.5),
            "b": lambda: [server.search(p, docs8_small, B, 0.5) for p in payloads],
            "c": lambda: server.search(payloads[0], docs8_full, B_full, 0.5)}
    orders = ("abc", "cba", "bca", "acb", "cab", "bac")
    t = {k: [] for k in runs}
    last = {}
    for i in range(warmup + steps):
        for k in orders[i % len(orders)]:
            sec, last[k] = timed(runs[k])
            if i >= warmup:
                t[k].append(sec)
    acc_a, below_a = client.decrypt_replies(last["a"])
    singles = [client.decrypt_reply(r) for r in last["b"]]
    parity = bool(all(torch.equal(acc_a[q], s[0]) and torch.equal(below_a[q], s[1]) for q, s in enumerate(singles)))
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs[:B]) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    exact = bool(np.array_equal(acc_a.cpu().numpy(), ref) and
                 np.array_equal(below_a.cpu().numpy(), (scores < 0.5).astype(np.int64)))
    acc_c, _ = client.decrypt_reply(last["c"])
    exact_c = bool(np.array_equal(acc_c.cpu().numpy(), Q.corpus_accumulate(oq, cq.s_e, n_bits, qs[0], docs)))
    med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
    out = {"Q": Qn, "B": B, "B_full": B_full, "ggsw_gadget": list(client.gadget),
           "pack_gadget": [client.pack_base_log, client.pack_level], "pack_margin_sigmas": client.margin,
           "a_search_many_ms": med["a"], "a_min_ms": min(t["a"]) * 1e3,
           "b_sequential_searches_ms": med["b"], "b_min_ms": min(t["b"]) * 1e3, "b_per_search_ms": med["b"] / Qn,
           "c_full_search_ms": med["c"], "c_min_ms": min(t["c"]) * 1e3,
           "ratio_a_over_b": med["a"] / med["b"], "meets_bar_a_over_b": med["a"] <= 0.5 * med["b"],
           "ratio_a_over_c": med["a"] / med["c"], "meets_bar_a_over_c": med["a"] <= 1.10 * med["c"],
           "small_search_over_full_search": med["b"] / Qn / med["c"],
           "reply_bytes": {"a": int(sum(r.nbytes for r in last["a"])), "b": int(sum(r.nbytes for r in last["b"])),
                           "c": int(last["c"].nbytes)},
           "query_bytes": int(sum(p.nbytes for p in payloads)),
           "parity_with_sequential": parity, "bit_exact": exact, "full_search_bit_exact": exact_c,
           "steps": steps, "warmup": warmup}
    out["leveled"] = private_leveled(server.engine, *client.gadget, D, steps, warmup, Qn, (B, B_full))
    out["meets_bar_leveled"] = bool(all(v["meets_bar"] for v in out["leveled"].values()
                                        if isinstance(v, dict) and "meets_bar" in v))
    # the feature stands on the two search_many bars; the bucket bar is reported beside them
    out["meets_bar"] = bool(out["meets_bar_a_over_b"] and out["meets_bar_a_over_c"] and parity and exact)
    server.engine.close()
    c.engine.close()
    return out


def private_rotated(cq, oq, D: int, n_bits: int, gens, steps: int, warmup: int, shapes=((8, 128), (1, 1024)),
                    leveled_only: bool = False) -> dict:
    """The both-private search after key rotations, one
    process. For every G of `gens`: an evaluation-only PrivateServer holding
    the newest generation's keys and a direct bridge key from each of G old
    generations, ALL documents old, in equal parts across the G generations
    (PrivateServer.search_resident, fhe_search_ggsws_gens_batch), against the
    unrotated PrivateServer.search_many of generation 0 over the same
    documents. The legs are interleaved in rotating order as rotated_gens
    does, host clock around each with a device synchronise (payload parse and
    upload, reply copies included); then a profiled pass for the
    "linear_ggsws" and "bridge" HIP-event buckets and one for the leveled step
    alone (Engine.linear_ggsws_gens between stream events, constants' upload
    included: the A/B of library builds reads it); and
    the parity of every leg's decrypted replies with the restatement.
    leveled_only (--no-end-to-end): the leveled step's pass alone, for the
    alternating-process A/B of library builds."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.private import PrivateClient, PrivateServer, unpack_any_query
    search_steps, search_warmup = (0, 0) if leveled_only else (steps, warmup)
    Gmax, Bmax = max(gens), max(B for _, B in shapes)
    c0 = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    clients = [PrivateClient(c0, count=1024, pack_seed=17, enc_seed=18)]
    for g in range(1, Gmax):     # generation g bridges from every generation before it: a store lives through them all
        clients.append(clients[-1].rotate(key_seed=5 + 2 * g, pack_seed=17 + g, bridge_seed=100 + 10 * g,
                                          noise_seed=6 + 2 * g, enc_seed=18 + g, bridge_from=list(clients)))
    keys = [c.eval_keys() for c in clients]
    plain = PrivateServer(keys[0], cq, c0.P0, scheme=c0.scheme)
    newest, newest_keys, servers = {}, {}, {}
    for G in gens:
        newest[G] = clients[G - 1].rotate(key_seed=50 + 2 * G, pack_seed=60 + G, bridge_seed=200 + 10 * G,
                                          noise_seed=70 + 2 * G, enc_seed=80 + G, bridge_from=clients[:G])
        newest_keys[G] = newest[G].eval_keys()
        servers[G] = PrivateServer(keys[0], cq, c0.P0, scheme=c0.scheme)
    _, docs = Q.make_corpus(D, Bmax, seed=21)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    first = newest[gens[0]]
    eng0 = servers[gens[0]].engine
    out = {"generations": list(gens), "ggsw_gadget": list(first.gadget), "bridge_gadget": list(first.bridge_gadget),
           "pack_gadget": [first.pack_base_log, first.pack_level], "pack_margin_sigmas": first.margin,
           "unrotated_pack_gadget": [clients[0].pack_base_log, clients[0].pack_level],
           "bridge_key_bytes_each": 8 * eng0.bridge_key_words(*first.bridge_gadget), "steps": steps, "warmup": warmup,
           "shapes": []}
    for Qn, B in shapes:
        qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
        plain_docs, _ = plain.pack_docs_many(clients[0].encrypt_docs(docs[:B]))
        plain_payloads = clients[0].encrypt_queries(qs)
        runs = {"unrotated": lambda: plain.search_many(plain_payloads, plain_docs, B, 0.5)}
        bundles, ends_of, blocks = {}, {}, {}
        for G in gens:
            if servers[G].generations:       # the shape before: a new host, again under generation 0's keys
                servers[G].engine.close()
                servers[G] = PrivateServer(keys[0], cq, c0.P0, scheme=c0.scheme)
            srv = servers[G]
            ends = [B * (g + 1) // G for g in range(G)]
            lo = [0] + ends[:-1]
            # the store's life: generation 0 loads its part; every later generation rekeys and appends its own;
            # the newest rekeys last, so ALL documents are old
            blocks[G] = [clients[g].encrypt_docs(docs[lo[g]:ends[g]]) for g in range(G)]
            srv.load(blocks[G][0])
            for g in range(1, G):
                srv.rekey(keys[g])
                srv.append(blocks[G][g])
            srv.rekey(newest_keys[G])
            assert srv.old_generations == srv.generations == [(clients[g].key_id, ends[g]) for g in range(G)]
            bundles[G] = newest[G].encrypt_queries_gens(qs, key_ids=[c.key_id for c in clients[:G]])
            ends_of[G] = ends
            runs[f"resident_g{G}"] = (lambda srv=srv, G=G: srv.search_resident(bundles[G], 0.5))
        names = list(runs)
        t = {k: [] for k in runs}
        last = {}
        for i in range(search_warmup + search_steps):
            for j in range(len(names)):                      # a rotating order: every leg in every position
                k = names[(i + j) % len(names)] if i % 2 == 0 else names[(i - j) % len(names)]
                sec, last[k] = timed(runs[k])
                if i >= search_warmup:
                    t[k].append(sec)
        ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs[:B]) for q in qs])
        scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
        exact = {}
        for k in (() if leveled_only else runs):
            who = clients[0] if k == "unrotated" else newest[int(k.rsplit("g", 1)[1])]
            acc, below = who.decrypt_replies(last[k])
            exact[k] = bool(np.array_equal(acc.cpu().numpy(), ref) and
                            np.array_equal(below.cpu().numpy(), (scores < 0.5).astype(np.int64)))
        # the HIP-event split, in passes of their own: three rounds of five searches per leg
        kerns = ("linear_ggsws", "bridge", "pack")
        split, kernels = {k: [] for k in runs}, {}
        for _ in range(0 if leveled_only else 3):
            for k in runs:
                eng = plain.engine if k == "unrotated" else servers[int(k.rsplit("g", 1)[1])].engine
                eng.profile(True)
                for kern in kerns:
                    eng.profile_read(kern)
                for _ in range(5):
                    runs[k]()
                torch.cuda.synchronize()
                split[k].append({kern: eng.profile_read(kern)["total_ms"] / 5 for kern in kerns})
                kernels[k] = eng.kernel_name("linear_ggsws")
                eng.profile(False)
        # the leveled step alone on each rotated server's operands: the "linear_ggsws" bucket per call
        leveled = {}
        for G in gens:
            srv = servers[G]
            eng = srv.engine
            items = []
            for g, block in enumerate(blocks[G]):      # rekey puts the bridge from generation g into slot g
                pls = [unpack_any_query(p) for p in bundles[G][clients[g].key_id]]
                operand, Bg = srv.pack_docs_many(block)
                items.append((g, eng.to_dev(np.concatenate([pl["ggsw"] for pl in pls])), operand, Bg))
            buf = eng.empty_big(Qn * B)
            per = []
            # stream events around the whole call: the loop build's scatters lie outside its buckets
            for i in range(warmup + steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.linear_ggsws_gens(items, *first.gadget, D, [0] * Qn, out=buf)
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    per.append(e0.elapsed_time(e1))
            leveled[f"g{G}"] = {"median_ms": statistics.median(per), "min_ms": min(per), "max_ms": max(per),
                                "kernel": eng.kernel_name("linear_ggsws")}
        if leveled_only:
            out["shapes"].append({"Q": Qn, "B": B, "ends": {f"g{G}": ends_of[G] for G in gens},
                                  "leveled_step_ms": leveled, "bit_exact": {}, "meets_bar": {}})
            continue
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        out["shapes"].append({
            "Q": Qn, "B": B, "ends": {f"g{G}": ends_of[G] for G in gens}, "ms_per_search": med,
            "min_ms": {k: min(v) * 1e3 for k, v in t.items()},
            "ratio_over_unrotated": {k: med[k] / med["unrotated"] for k in med},
            "meets_bar": {k: med[k] <= 1.10 * med["unrotated"] for k in med if k != "unrotated"},
            "event_ms_per_search": {k: {kern: statistics.median(r[kern] for r in v) for kern in kerns}
                                    for k, v in split.items()},
            "linear_ggsws_kernel": kernels, "leveled_step_ms": leveled,
            "query_bytes": {k: int(sum(p.nbytes for v in bundles[int(k.rsplit("g", 1)[1])].values() for p in v))
                            if k != "unrotated" else int(sum(p.nbytes for p in plain_payloads)) for k in runs},
            "bit_exact": exact})
    out["bit_exact"] = all(all(s["bit_exact"].values()) for s in out["shapes"])
    out["meets_bar"] = all(all(s["meets_bar"].values()) for s in out["shapes"])
    for srv in [plain] + list(servers.values()):
        srv.engine.close()
    for c in clients + list(newest.values()):
        c.corpus.engine.close()
    return out


def seeded_private(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Qn: int = 8, B: int = 128,
                   load_sizes=(1024, 65536)) -> dict:
    """The both-private search on seeded payloads against the
    full form, one process, one server. Payload bytes; per corpus size the load
    (PrivateServer.pack_docs_many: parse, host-to-device copy, operand kernel)
    seeded against full form, interleaved in alternating order, and the
    operand step alone on resident inputs (HIP events); then
    PrivateServer.search_many, Qn queries x B documents, three legs
    interleaved in rotating order: (a) full form, (b) seeded, (c) full form
    again, whose spread against (a) is the margin the ratio b / a is read
    with; and k_expand_ggsw_seeded alone (HIP events). The seeded client's
    words are the full-form client's (one key for masks and noise, a test
    arrangement), so the replies are compared word for word."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp import private as P
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    full = P.PrivateClient(c, count=Qn * B, pack_seed=17, enc_seed=18)
    seeded = P.PrivateClient(c, count=Qn * B, pack_seed=17, enc_seed=18, seeded=True)
    seeded._mask_key = full._enc_key.copy()      # measurement only: the two clients' ciphertext words coincide
    server = P.PrivateServer(full.eval_keys(), cq, c.P0, scheme=c.scheme)
    eng = server.engine

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    out = {"Q": Qn, "B": B, "ggsw_gadget": list(full.gadget), "steps": steps, "warmup": warmup, "load": {}}
    same = True
    for n, Bl in enumerate(load_sizes):
        _, docs = Q.make_corpus(D, Bl, seed=21)
        id0 = (n + 1) << 32                      # every block its own ids: the server refuses a repeat
        blocks = {"full": full.encrypt_docs(docs, id0=id0), "seeded": seeded.encrypt_docs(docs, id0=id0)}
        t = {k: [] for k in blocks}
        tk = {k: [] for k in blocks}
        last = {}
        bl_f, bl_s = P.unpack_doc_block(blocks["full"]), P.unpack_doc_block_seeded(blocks["seeded"])
        d_f, d_s = eng.to_dev(bl_f["glwe"]), eng.to_dev(bl_s["body"])
        kern = {"full": lambda: eng.pack_docs_glwe_queries(d_f, Bl, D, server.base_log, server.level),
                "seeded": lambda: eng.pack_docs_glwe_seeded(d_s, bl_s["id0"], bl_s["mask_key"], Bl, D, server.base_log,
                                                            server.level, queries=True)}
        for i in range(warmup + steps):
            for k in (("full", "seeded") if i % 2 == 0 else ("seeded", "full")):
                sec, (last[k], _) = timed(lambda k=k: server.pack_docs_many(blocks[k]))
                ms, _ = events(kern[k])
                if i >= warmup:
                    t[k].append(sec)
                    tk[k].append(ms)
        same = same and bool(torch.equal(last["full"], last["seeded"]))
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        medk = {k: statistics.median(v) for k, v in tk.items()}
        out["load"][str(Bl)] = {
            "block_bytes": {k: int(b.nbytes) for k, b in blocks.items()},
            "pack_docs_many_ms": med, "pack_docs_many_min_ms": {k: min(v) * 1e3 for k, v in t.items()},
            "operand_step_alone_ms": medk, "ratio_seeded_over_full": med["seeded"] / med["full"],
            "ratio_operand_step_seeded_over_full": medk["seeded"] / medk["full"],
            "seeded_no_slower": med["seeded"] <= med["full"]}
        del d_f, d_s, last
    _, docs = Q.make_corpus(D, B, seed=21)
    qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
    docs_op, _ = server.pack_docs_many(seeded.encrypt_docs(docs, id0=5000))
    pay = {"full": full.encrypt_queries(qs, id0=7000), "seeded": seeded.encrypt_queries(qs, id0=7000)}
    runs = {"a": lambda: server.search_many(pay["full"], docs_op, B, 0.5),
            "b": lambda: server.search_many(pay["seeded"], docs_op, B, 0.5),
            "c": lambda: server.search_many(pay["full"], docs_op, B, 0.5)}
    orders = ("abc", "cba", "bca", "acb", "cab", "bac")
    t = {k: [] for k in runs}
    last = {}
    for i in range(warmup + steps):
        for k in orders[i % len(orders)]:
            sec, last[k] = timed(runs[k])
            if i >= warmup:
                t[k].append(sec)
    med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
    pls = [P.unpack_ggsw_query_seeded(p) for p in pay["seeded"]]
    bodies = eng.to_dev(np.concatenate([pl["body"] for pl in pls]))
    ids = [pl["id0"] for pl in pls]
    ex = [events(lambda: eng.expand_ggsws_seeded(bodies, ids, server.base_log, server.level, pls[0]["mask_key"]))[0]
          for _ in range(warmup + steps)][warmup:]
    acc, below = full.decrypt_replies(last["b"])
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs) for q in qs])
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    exact = bool(np.array_equal(acc.cpu().numpy(), ref) and
                 np.array_equal(below.cpu().numpy(), (scores < 0.5).astype(np.int64)))
    words = bool(len(last["a"]) == len(last["b"]) and all(np.array_equal(x, y) for x, y in zip(last["a"], last["b"])))
    spread = abs(med["c"] / med["a"] - 1.0)
    out.update({
        "query_bytes": {k: int(p[0].nbytes) for k, p in pay.items()},
        "a_full_ms": med["a"], "b_seeded_ms": med["b"], "c_full_again_ms": med["c"],
        "min_ms": {k: min(v) * 1e3 for k, v in t.items()},
        "ratio_seeded_over_full": med["b"] / med["a"], "full_against_full_spread": spread,
        "seeded_within_spread": abs(med["b"] / med["a"] - 1.0) <= spread,
        "expand_ggsw_seeded_ms": statistics.median(ex), "expand_ggsw_seeded_min_ms": min(ex),
        "operands_equal": same, "replies_equal_word_for_word": words, "bit_exact": exact})
    server.engine.close()
    c.engine.close()
    return out


def both_private(cq, oq, B: int, D: int, n_bits: int, steps: int, warmup: int) -> dict:
    """fhe_compare_ggsw_batch against fhe_compare_query_batch on one context,
    interleaved in alternating order."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp.corpus import EncryptedCorpus
    from fheicp.private import PrivateClient, unpack_doc_block, unpack_ggsw_query
    from fheicp.query import EncryptedQuerySearch
    c = EncryptedCorpus(cq).compile(key_seed=5, device=0, noise_seed=6)
    eng = c.engine
    single = EncryptedQuerySearch(c)
    client = PrivateClient(c, count=B, pack_seed=17, enc_seed=18)
    beta, L = client.gadget
    q, docs = Q.make_corpus(D, B, seed=21)
    docs8_q = single.pack_docs(docs)
    docs8_g = eng.pack_docs_glwe(eng.to_dev(unpack_doc_block(client.encrypt_docs(docs))["glwe"]), B, D, beta, L)
    payload_q, payload_g = single.encrypt_query(q), client.encrypt_query(q)
    _, cst, T = single.plan(0.5)
    eng.set_msg_bits(c.P0)
    eng.profile(True)
    t_query, t_ggsw, t_lin = [], [], []

    def run_query():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = single.compare(payload_q, docs8_q, B, 0.5)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def run_ggsw():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pl = unpack_ggsw_query(payload_g)
        out = eng.compare_ggsw(eng.to_dev(pl["ggsw"]), beta, L, docs8_g, B, D, cst, T)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for i in range(warmup + steps):
        if i % 2:
            (tq, res_q), (tg, res_g) = run_query(), run_ggsw()
        else:
            (tg, res_g), (tq, res_q) = run_ggsw(), run_query()
        lin = eng.profile_read("linear_ggsw")
        assert lin["launches"] == 1
        eng.profile_read("linear_query")
        if i >= warmup:
            t_query.append(tq)
            t_ggsw.append(tg)
            t_lin.append(lin["total_ms"])
    eng.profile(False)
    ref = Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs)
    scores = np.float64(Q.corpus_out_scale(oq, cq.s_e)) * ref.astype(np.float64)
    parity = bool(torch.equal(res_g[0], res_q[0]) and torch.equal(res_g[1], res_q[1]))
    exact = bool(np.array_equal(res_g[0].cpu().numpy(), ref) and
                 np.array_equal(res_g[1].cpu().numpy(), (scores < 0.5).astype(np.int64)))
    q_ms, g_ms = statistics.median(t_query) * 1e3, statistics.median(t_ggsw) * 1e3
    p = c.scheme
    n1 = (p.k + 1) * p.N
    out = {"compare_ggsw_ms": g_ms, "compare_ggsw_min_ms": min(t_ggsw) * 1e3, "compare_query_ms": q_ms,
           "compare_query_min_ms": min(t_query) * 1e3, "ratio_ggsw_over_query": g_ms / q_ms,
           "meets_bar": g_ms <= 1.10 * q_ms, "linear_ggsw_ms": statistics.median(t_lin),
           "linear_ggsw_min_ms": min(t_lin), "kernel": eng.kernel_name("linear_ggsw"), "ggsw_gadget": [beta, L],
           "ggsw_bytes": int(payload_g.nbytes), "plane_bytes": n1 * L * n1 * 8,
           "doc_glwes": eng.doc_glwes(B, D), "parity_with_compare_query": parity, "bit_exact": exact,
           "steps": steps, "warmup": warmup}
    c.engine.close()
    return out


def seeded_keys(cq, oq, D: int, n_bits: int, steps: int, warmup: int, Qn: int = 2, B: int = 64) -> dict:
    """Seeded evaluation keys against the full form, one
    process: sizes of one client's set in both forms, import_eval_keys of each
    form on one evaluation-only context (interleaved, alternating order), and
    one search per server kind from either form, replies word for word."""
    import numpy as np
    import torch
    from oracle import quant_ref as Q
    from fheicp import private as P
    from fheicp.corpus import EncryptedCorpus
    from fheicp.engine import Engine
    from fheicp.query import QueryClient, QueryServer
    from fheicp.stored import CorpusClient, CorpusServer

    def compiled(i):
        return EncryptedCorpus(cq).compile(key_seed=5 + i, device=0, noise_seed=6 + i, seeded_keys=True,
                                           key_mask_seed=50 + 100 * i)

    def sizes(d):
        return {k: int(np.asarray(v).nbytes) for k, v in d.items()}

    c = compiled(0)
    client = QueryClient(c, count=Qn * B, pack_seed=17)
    ds, df = client.eval_keys(), client.eval_keys(seeded=False)
    out = {"Q": Qn, "B": B, "steps": steps, "warmup": warmup, "pack_gadget": [int(x) for x in ds["pack_gadget"]],
           "bytes": {"seeded": sizes(ds), "full": sizes(df)}}
    out["bytes"]["seeded_total"] = sum(out["bytes"]["seeded"].values())
    out["bytes"]["full_total"] = sum(out["bytes"]["full"].values())
    out["bytes"]["ratio_seeded_over_full"] = out["bytes"]["seeded_total"] / out["bytes"]["full_total"]
    eng = Engine(c.scheme, 0)
    forms = {"seeded": ds, "full": df}
    t = {k: [] for k in forms}
    for i in range(warmup + steps):
        for k in (("full", "seeded") if i % 2 == 0 else ("seeded", "full")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.import_eval_keys(forms[k])
            torch.cuda.synchronize()
            if i >= warmup:
                t[k].append(time.perf_counter() - t0)
    eng.close()
    med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
    out["import_eval_keys_ms"] = med
    out["import_eval_keys_min_ms"] = {k: min(v) * 1e3 for k, v in t.items()}
    out["import_ratio_seeded_over_full"] = med["seeded"] / med["full"]
    out["seeded_import_faster"] = med["seeded"] < med["full"]

    _, docs = Q.make_corpus(D, B, seed=21)
    qs = np.stack([Q.make_corpus(D, 1, seed=100 + i)[0] for i in range(Qn)])
    ref = np.stack([Q.corpus_accumulate(oq, cq.s_e, n_bits, q, docs) for q in qs])
    out["search"] = {}

    def record(name, replies, decrypt):
        same = len(replies[0]) == len(replies[1]) and all(np.array_equal(a, b) for a, b in zip(*replies))
        acc, _ = decrypt(replies[0])
        out["search"][name] = {"replies_equal_word_for_word": bool(same),
                               "bit_exact": bool(np.array_equal(acc.cpu().numpy(), ref))}

    payloads, replies = client.encrypt_queries(qs), []
    for keys in (ds, df):
        server = QueryServer(keys, cq, c.P0, scheme=c.scheme)
        replies.append(server.search_many(payloads, server.pack_docs(docs), B, 0.5))
        server.engine.close()
    record("QueryServer", replies, client.decrypt_replies)
    c.engine.close()

    c = compiled(1)
    client = CorpusClient(c, count=Qn * B, pack_seed=18)
    stored, replies = client.encrypt_docs(docs), []
    for keys in (client.eval_keys(), client.eval_keys(seeded=False)):
        server = CorpusServer(keys, cq, c.P0, c.mask_key, scheme=c.scheme)
        server.load(*stored)
        replies.append(server.search_many(qs, 0.5))
        server.engine.close()
    record("CorpusServer", replies, client.decrypt_replies)
    c.engine.close()

    c = compiled(2)
    client = P.PrivateClient(c, count=Qn * B, pack_seed=19, enc_seed=20)
    block, payloads, replies = client.encrypt_docs(docs), client.encrypt_queries(qs), []
    for keys in (client.eval_keys(), client.eval_keys(seeded=False)):
        server = P.PrivateServer(keys, cq, c.P0, scheme=c.scheme)
        docs_op, Bn = server.pack_docs_many(block)
        replies.append(server.search_many(payloads, docs_op, Bn, 0.5))
        server.engine.close()
    record("PrivateServer", replies, client.decrypt_replies)
    c.engine.close()
    out["bit_exact"] = all(v["bit_exact"] and v["replies_equal_word_for_word"] for v in out["search"].values())
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 768])
    ap.add_argument("--n-bits", type=int, nargs="+", default=[6, 8])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-end-to-end", action="store_true",
                    help="the leveled step only (kernel traces: no keygen, no sign extraction)")
    ap.add_argument("--two-party", action="store_true",
                    help="the two-party search (evaluation-only server, packed reply) against the single-party "
                         "compare, --launches interleaved steps after --warmup")
    ap.add_argument("--both-private", action="store_true",
                    help="the both-private compare (GGSW query, GLWE documents) against the private-query "
                         "compare, --launches interleaved steps after --warmup")
    ap.add_argument("--multi-query", action="store_true",
                    help="several queries in one batched call (16-dim, n_bits 6, two-party): search_many with "
                         "Q = 8, B = 128 against eight sequential searches and one B = 1024 search, 24 "
                         "interleaved steps after 4 warm-up; writes profiles/r11/multi_query.json")
    ap.add_argument("--stored-queries", action="store_true",
                    help="the stored-ciphertext search for several clear queries (16-dim, n_bits 6, two-party): "
                         "CorpusServer.search_many with Q = 8, B = 128 against eight sequential searches and one "
                         "B = 1024 compare, and the batched leveled step against eight single calls at B = 128 "
                         "and 1024; 24 interleaved steps after 4 warm-up; writes profiles/r12/stored_queries.json "
                         "(with --no-end-to-end: the leveled step only, no keys)")
    ap.add_argument("--private-queries", action="store_true",
                    help="the both-private search for several GGSW queries (16-dim, n_bits 6, two-party): "
                         "PrivateServer.search_many with Q = 8, B = 128 against eight sequential searches and one "
                         "B = 1024 search, and the batched leveled step against eight single calls at B = 128 "
                         "and 1024; 24 interleaved steps after 4 warm-up; writes profiles/r13/private_queries.json "
                         "(with --no-end-to-end: the leveled step only, no keys)")
    ap.add_argument("--tenants", action="store_true",
                    help="several key holders in one batched call (16-dim, n_bits 6, two-party): QueryHub.search_many "
                         "for 8 tenants x (Q = 1, B = 128) against the eight QueryServer.search calls and one "
                         "tenant's B = 1024 search, 24 interleaved steps after 4 warm-up, with the HIP-event split "
                         "per run; writes profiles/r14/tenants.json")
    ap.add_argument("--rotated", action="store_true",
                    help="the stored-ciphertext search after a key rotation (16-dim, n_bits 6, two-party, DESIGN.md "
                         "§8.12): CorpusServer.search_many at 8 queries x 128 documents and 1 x 1024 with every, half "
                         "and none of the documents old-generation (bridged), 24 interleaved steps after 4 warm-up, "
                         "with the bridge bucket's HIP-event time; writes profiles/r15/rotated.json")
    ap.add_argument("--generations", type=int, default=1, metavar="G",
                    help="with --stored-tenants: every tenant's documents in G old generations, the hub with "
                         "rotation_schedules (DESIGN.md §8.18; writes profiles/r21/stored_tenants_gens.json). "
                         "With --rotated: G old generations resident (DESIGN.md §8.17), legs \"G old generations in "
                         "equal parts\", \"all one old generation\" and \"none old\" with the bridge bucket's "
                         "HIP-event time; writes profiles/r20/rotated_gens.json. Default 1: --rotated as it was")
    ap.add_argument("--private-rotated", action="store_true",
                    help="the both-private search after key rotations (16-dim, n_bits 6, two-party, DESIGN.md §8.19): "
                         "PrivateServer.search_resident with all documents old, in equal parts across G old "
                         "generations, for G in {1, 3} (or the one G of --generations), against the unrotated "
                         "search_many of the same process, at 8 queries x 128 documents and 1 x 1024, 24 interleaved "
                         "steps after 4 warm-up, with the \"linear_ggsws\" and \"bridge\" buckets' HIP-event times "
                         "and the leveled step alone; writes profiles/r22/private_rotated.json")
    ap.add_argument("--plain-first", action="store_true",
                    help="with --stored-tenants --generations 1: build and run the default hub before the "
                         "rotation_schedules hub (the order's own effect on the comparison)")
    ap.add_argument("--stored-tenants", action="store_true",
                    help="several key holders' stored documents in one batched call (16-dim, n_bits 6, two-party, "
                         "DESIGN.md §8.13): CorpusHub.search_many for 8 tenants x (Q = 1, B = 128) against the eight "
                         "CorpusServer.search calls and one tenant's B = 1024 search, 24 interleaved steps after 4 "
                         "warm-up, with the HIP-event split per run, then again with every tenant rotated (all "
                         "documents old); writes profiles/r16/stored_tenants.json")
    ap.add_argument("--private-tenants", action="store_true",
                    help="measure several key holders' both-private searches in one batched call (two-party, "
                         "DESIGN.md §8.14): PrivateHub.search_many for 8 tenants x (Q = 1, B = 128) against the eight "
                         "PrivateServer.search calls and one tenant's B = 1024 search, 24 interleaved steps after 4 "
                         "warm-up, with the HIP-event split per run, then the grouped leveled step against the "
                         "tenants' own calls; writes profiles/r17/private_tenants.json")
    ap.add_argument("--seeded-private", action="store_true",
                    help="the both-private search on seeded payloads (DESIGN.md §8.15) at 16-dim n_bits 6: payload "
                         "bytes, the corpus load (pack_docs_many, copy included) seeded against full form at B = 1024 "
                         "and 65536 with the operand step alone, search_many 8 queries x 128 documents seeded against "
                         "two full-form series, and k_expand_ggsw_seeded alone; 24 interleaved steps after 4 warm-up; "
                         "writes profiles/r18/seeded_private.json")
    ap.add_argument("--seeded-keys", action="store_true",
                    help="seeded evaluation keys (DESIGN.md §8.16) at 16-dim n_bits 6: bytes of both forms of one "
                         "client's key set, import_eval_keys of each form interleaved (8 steps after 2 warm-up), one "
                         "search per server kind from either form with the replies compared word for word; writes "
                         "profiles/r19/seeded_keys.json")
    ap.add_argument("--tenant-shape", type=int, nargs=2, default=[8, 128], metavar=("T", "B"),
                    help="--tenants / --stored-tenants / --private-tenants: T tenants of B documents each (default 8 128)")
    ap.add_argument("--out", default=None, help="default profiles/query_bench.json "
                                                "(--multi-query: profiles/r11/multi_query.json, "
                                                "--stored-queries: profiles/r12/stored_queries.json, "
                                                "--private-queries: profiles/r13/private_queries.json, "
                                                "--seeded-private: profiles/r18/seeded_private.json, "
                                                "--seeded-keys: profiles/r19/seeded_keys.json)")
    a = ap.parse_args()
    a.generations_given = any(x == "--generations" or x.startswith("--generations=") for x in sys.argv[1:])
    if a.out is None:
        a.out = str(REPO / "profiles" / ("r22/private_rotated.json" if a.private_rotated else
                                         "r19/seeded_keys.json" if a.seeded_keys else
                                         "r18/seeded_private.json" if a.seeded_private else
                                         "r17/private_tenants.json" if a.private_tenants else
                                         "r21/stored_tenants_gens.json" if a.stored_tenants and a.generations_given
                                         else "r16/stored_tenants.json" if a.stored_tenants else
                                         "r20/rotated_gens.json" if a.rotated and a.generations > 1 else
                                         "r15/rotated.json" if a.rotated else
                                         "r14/tenants.json" if a.tenants else
                                         "r11/multi_query.json" if a.multi_query else
                                         "r12/stored_queries.json" if a.stored_queries else
                                         "r13/private_queries.json" if a.private_queries else "query_bench.json"))
    if a.launches < 20:
        ap.error("--launches must be >= 20 (the medians compared are of at least 20 launches)")
    import torch
    if not torch.cuda.is_available():
        print("query_bench needs a GPU: nothing measured", file=sys.stderr)
        return 2
    from fheicp.engine import Engine
    from fheicp.params import params_for_bits
    if a.private_rotated:
        from fheicp import _lib
        if not 1 <= a.generations <= _lib.BRIDGE_SLOTS:
            ap.error(f"--generations is 1 to {_lib.BRIDGE_SLOTS}")
        cq, oq = corpus_quant(16, 6)
        gens = (a.generations,) if a.generations_given else (1, 3)
        pr = private_rotated(cq, oq, 16, 6, gens, steps=24, warmup=4, leveled_only=a.no_end_to_end)
        res = {"bench": "query_bench --private-rotated" + (f" --generations {a.generations}" if a.generations_given
                                                            else ""),
               "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6, "P0": cq.worst_msg_bits(),
               "build": _lib.lib().fhe_build_info().decode(), "lib": Path(_lib.LIB_PATH).name, "private_rotated": pr,
               "bit_exact": pr["bit_exact"], "meets_bar": pr["meets_bar"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.seeded_keys:
        cq, oq = corpus_quant(16, 6)
        sk = seeded_keys(cq, oq, 16, 6, steps=8, warmup=2)
        from fheicp import _lib
        res = {"bench": "query_bench --seeded-keys", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": cq.worst_msg_bits(), "build": _lib.lib().fhe_build_info().decode(), "seeded_keys": sk,
               "bit_exact": bool(sk["bit_exact"])}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.seeded_private:
        cq, oq = corpus_quant(16, 6)
        sp = seeded_private(cq, oq, 16, 6, steps=24, warmup=4)
        from fheicp import _lib
        res = {"bench": "query_bench --seeded-private", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": cq.worst_msg_bits(), "build": _lib.lib().fhe_build_info().decode(), "seeded_private": sp,
               "bit_exact": bool(sp["bit_exact"] and sp["operands_equal"] and sp["replies_equal_word_for_word"])}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.rotated and a.generations > 1:
        from fheicp import _lib
        if a.generations > _lib.BRIDGE_SLOTS:
            ap.error(f"--generations is at most {_lib.BRIDGE_SLOTS}")
        cq, oq = corpus_quant(16, 6)
        ro = rotated_gens(cq, oq, 16, 6, a.generations, steps=24, warmup=4)
        res = {"bench": f"query_bench --rotated --generations {a.generations}", "device": torch.cuda.get_device_name(0),
               "D": 16, "n_bits": 6, "P0": cq.worst_msg_bits(), "build": _lib.lib().fhe_build_info().decode(),
               "lib": Path(_lib.LIB_PATH).name, "rotated_gens": ro, "bit_exact": ro["bit_exact"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.rotated:
        cq, oq = corpus_quant(16, 6)
        ro = rotated(cq, oq, 16, 6, steps=24, warmup=4)
        from fheicp import _lib
        res = {"bench": "query_bench --rotated", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": cq.worst_msg_bits(), "build": _lib.lib().fhe_build_info().decode(), "rotated": ro,
               "bit_exact": ro["bit_exact"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.private_tenants:
        cq, oq = corpus_quant(16, 6)
        tn = private_tenants(cq, oq, 16, 6, steps=24, warmup=4, Tn=a.tenant_shape[0], B=a.tenant_shape[1])
        res = {"bench": "query_bench --private-tenants", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": cq.worst_msg_bits(), "private_tenants": tn, "meets_bar": tn["meets_bar"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.stored_tenants and a.generations_given:
        from fheicp import _lib
        if not 1 <= a.generations <= _lib.BRIDGE_SLOTS:
            ap.error(f"--generations is 1 to {_lib.BRIDGE_SLOTS}")
        cq, oq = corpus_quant(16, 6)
        tg = stored_tenants_gens(cq, oq, 16, 6, a.generations, steps=24, warmup=4, Tn=a.tenant_shape[0],
                                 B=a.tenant_shape[1], plain_first=a.plain_first)
        res = {"bench": f"query_bench --stored-tenants --generations {a.generations}",
               "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6, "P0": cq.worst_msg_bits(),
               "stored_tenants_gens": tg, "bit_exact": tg["bit_exact"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.stored_tenants:
        cq, oq = corpus_quant(16, 6)
        tn = stored_tenants(cq, oq, 16, 6, steps=24, warmup=4, Tn=a.tenant_shape[0], B=a.tenant_shape[1])
        res = {"bench": "query_bench --stored-tenants", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": cq.worst_msg_bits(), "stored_tenants": tn, "meets_bar": tn["meets_bar"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.tenants:
        cq, oq = corpus_quant(16, 6)
        tn = tenants(cq, oq, 16, 6, steps=24, warmup=4, Tn=a.tenant_shape[0], B=a.tenant_shape[1])
        res = {"bench": "query_bench --tenants", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": cq.worst_msg_bits(), "tenants": tn, "meets_bar": tn["meets_bar"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.multi_query:
        cq, oq = corpus_quant(16, 6)
        mq = multi_query(cq, oq, 16, 6, steps=24, warmup=4)
        res = {"bench": "query_bench --multi-query", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": cq.worst_msg_bits(), "multi_query": mq, "meets_bar": mq["meets_bar"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.stored_queries:
        cq, oq = corpus_quant(16, 6)
        P0 = cq.worst_msg_bits()
        if a.no_end_to_end:
            eng = Engine(params_for_bits(P0), 0)
            sq = {"leveled": stored_leveled(eng, 16, steps=24, warmup=4)}
            sq["meets_bar"] = all(v["meets_bar"] for k, v in sq["leveled"].items() if k != "kernel")
            eng.close()
        else:
            sq = stored_queries(cq, oq, 16, 6, steps=24, warmup=4)
        from fheicp import _lib
        res = {"bench": "query_bench --stored-queries", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": P0, "build": _lib.lib().fhe_build_info().decode(), "stored_queries": sq,
               "meets_bar": sq["meets_bar"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    if a.private_queries:
        cq, oq = corpus_quant(16, 6)
        P0 = cq.worst_msg_bits()
        if a.no_end_to_end:
            eng = Engine(params_for_bits(P0), 0)
            pq = {"leveled": private_leveled(eng, 7, 6, 16, steps=24, warmup=4)}
            pq["meets_bar_leveled"] = all(v["meets_bar"] for v in pq["leveled"].values()
                                          if isinstance(v, dict) and "meets_bar" in v)
            pq["meets_bar"] = pq["meets_bar_leveled"]
            eng.close()
        else:
            pq = private_queries(cq, oq, 16, 6, steps=24, warmup=4)
        from fheicp import _lib
        res = {"bench": "query_bench --private-queries", "device": torch.cuda.get_device_name(0), "D": 16, "n_bits": 6,
               "P0": P0, "build": _lib.lib().fhe_build_info().decode(), "private_queries": pq,
               "meets_bar": pq["meets_bar"]}
        line = json.dumps(res)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
        print(line)
        return 0
    shapes = []
    for D in a.dims:
        for nb in a.n_bits:
            cq, oq = corpus_quant(D, nb)
            P0 = cq.worst_msg_bits()
            if a.both_private:
                from fheicp.private import plan_gadget
                row = {"B": a.batch, "D": D, "n_bits": nb, "P0": P0, "both_private": None}
                if P0 <= MAX_BITS:
                    try:
                        plan_gadget(params_for_bits(P0), cq)
                    except ValueError as e:          # no gadget at this width: recorded, not measured
                        row["no_gadget"] = str(e)
                    else:
                        row["both_private"] = both_private(cq, oq, a.batch, D, nb, a.launches, a.warmup)
                row["meets_bar"] = row["both_private"] is None or row["both_private"]["meets_bar"]
                shapes.append(row)
                continue
            if a.two_party:
                row = {"B": a.batch, "D": D, "n_bits": nb, "P0": P0,
                       "two_party": two_party(cq, oq, a.batch, D, nb, a.launches, a.warmup) if P0 <= MAX_BITS else None}
                row["meets_bar"] = row["two_party"] is None or row["two_party"]["meets_bar"]
                shapes.append(row)
                continue
            # the leveled step's shape is B x D x (kN + 1): the same for every planned width
            eng = Engine(params_for_bits(min(P0, MAX_BITS)), 0)
            row = {"B": a.batch, "D": D, "n_bits": nb, "P0": P0}
            row.update(leveled(eng, a.batch, D, nb, a.launches, a.warmup))
            eng.close()
            row["end_to_end"] = (end_to_end(cq, oq, a.batch, D, nb, a.reps)
                                 if P0 <= MAX_BITS and not a.no_end_to_end else None)
            row["meets_bar"] = row["linear_query_ms"] <= row["linear_seeded_ms"]
            shapes.append(row)
    res = {"bench": "query_bench", "device": torch.cuda.get_device_name(0), "copy_bw_bytes_per_s": COPY_BW,
           "shapes": shapes, "meets_bar": all(r["meets_bar"] for r in shapes)}
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
