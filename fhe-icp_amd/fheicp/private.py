"""Both-private search: a GGSW-encrypted query against GLWE-encrypted documents.

The fourth deployment shape: the host that stores and scores
sees neither the documents nor the query.

  * the client quantizes documents with the corpus quantizer,
    ``dq = E.quant(d)`` (fheicp.corpus.CorpusQuant), and encrypts S = N // D
    of them per GLWE at the worst-case width P0, feature j of document i at
    coefficient i D + j (fhe_encrypt_packed_batch);
  * it quantizes a query the same way, folds it into the model's weights,
    ``W_j = q_w[j] * qq_j``, and sends one GGSW of ``Q = sum_j W_j X^-j``
    (fhe_encrypt_ggsw) with the gadget of params.extprod_plan;
  * the server decomposes the documents once (fhe_glwe_docs_pack) and
    computes ``acc_b = sum_j W_j * dq[b, j] + q_b'`` as one exact external
    product modulo 2^64 on the i8 matrix cores, then the sign extraction of
    ``acc - T`` and the packed replies of the two-party private query
    (fhe_search_ggsw_batch); it holds evaluation keys, the CorpusQuant and P0.

Several queries of one key holder go in one pass:
``PrivateClient.encrypt_queries`` gives each query its own stream-id range,
``PrivateServer.pack_docs_many`` makes the batched document operand and
``search_many`` answers with fheicp.query's version-2 replies
(fhe_search_ggsws_batch: the product transposed, no Toeplitz operand).

The expected values are the bilinear restatement of fheicp.corpus
(oracle/quant_ref.py, ``corpus_*``); reply format and packing plan are
fheicp.query's.

Query payload (uint64 vector):
    [QUERY_MAGIC, 1, D, P0, base_log | level << 32, N | k << 32,
     GGSW words [c][l][component][coef]]
Document block (uint64 vector):
    [DOCS_MAGIC, 1, B, D, P0, N | k << 32, ceil(B / (N // D)) GLWEs of (k+1)N words]
"""
from __future__ import annotations

import os

import numpy as np

from .corpus import EncryptedCorpus
from .query import QueryClient, QueryServer, pack_reply

QUERY_MAGIC = int.from_bytes(b"FHEICPGQ", "little")
DOCS_MAGIC = int.from_bytes(b"FHEICPGD", "little")
HEADER_WORDS = 6


def pack_ggsw_query(ggsw, D: int, P0: int, base_log: int, level: int, N: int, k: int) -> np.ndarray:
    g = np.asarray(ggsw, dtype=np.uint64).reshape(-1)
    head = np.array([QUERY_MAGIC, 1, D, P0, int(base_log) | (int(level) << 32), int(N) | (int(k) << 32)], np.uint64)
    return np.concatenate([head, g])


def unpack_ggsw_query(arr) -> dict:
    a = np.asarray(arr)
    if a.dtype != np.uint64 or a.ndim != 1 or a.size < HEADER_WORDS or int(a[0]) != QUERY_MAGIC:
        raise ValueError("not an fheicp GGSW query payload")
    if int(a[1]) != 1:
        raise ValueError(f"unsupported GGSW query payload version {int(a[1])}")
    base_log, level = int(a[4]) & 0xFFFFFFFF, int(a[4]) >> 32
    N, k = int(a[5]) & 0xFFFFFFFF, int(a[5]) >> 32
    if a.size != HEADER_WORDS + (k + 1) * level * (k + 1) * N:
        raise ValueError("GGSW query payload size does not match its gadget and parameters")
    return {"D": int(a[2]), "P0": int(a[3]), "base_log": base_log, "level": level, "N": N, "k": k,
            "ggsw": a[HEADER_WORDS:].copy()}


# ------------------------------------------------------ batches of queries --
# Several GGSW queries of one key holder answered in one pass (DESIGN.md
# §8.10): a batch is a list of the payloads above, no new format.
def ggsw_id_span(k: int, level: int) -> int:
    """Stream ids one GGSW consumes: (k+1) L k mask ids from its id0 on (the
    (k+1) L noise ids are the first of the same range, under another tag)."""
    return (int(k) + 1) * int(level) * int(k)


def ggsw_query_ids(id0: int, Q: int, k: int, level: int) -> list:
    """id0 of each of Q queries of one batch: query q takes
    [id0 + q span, id0 + (q + 1) span) modulo 2^64, span = ggsw_id_span."""
    span = ggsw_id_span(k, level)
    return [(int(id0) + q * span) % (1 << 64) for q in range(int(Q))]


def check_ggsw_batch(pls) -> None:
    """The unpacked GGSW payloads of one batch agree in D, P0, gadget, N and
    k. ValueError names the offending query."""
    if not pls:
        raise ValueError("an empty batch of queries")
    first = pls[0]
    for i, pl in enumerate(pls[1:], 1):
        for field, what in (("D", "dimension D"), ("P0", "width P0"), ("base_log", "gadget base_log"),
                            ("level", "gadget level"), ("N", "polynomial size N"), ("k", "GLWE dimension k")):
            if pl[field] != first[field]:
                raise ValueError(f"query {i}: {what} {pl[field]} differs from query 0's {first[field]}")


def pack_doc_block(glwe, B: int, D: int, P0: int, N: int, k: int) -> np.ndarray:
    g = np.asarray(glwe, dtype=np.uint64).reshape(-1)
    head = np.array([DOCS_MAGIC, 1, B, D, P0, int(N) | (int(k) << 32)], np.uint64)
    return np.concatenate([head, g])


def unpack_doc_block(arr) -> dict:
    a = np.asarray(arr)
    if a.dtype != np.uint64 or a.ndim != 1 or a.size < HEADER_WORDS or int(a[0]) != DOCS_MAGIC:
        raise ValueError("not an fheicp GLWE document block")
    if int(a[1]) != 1:
        raise ValueError(f"unsupported document block version {int(a[1])}")
    B, D = int(a[2]), int(a[3])
    N, k = int(a[5]) & 0xFFFFFFFF, int(a[5]) >> 32
    if not 0 < D <= N:
        raise ValueError(f"document block of D = {D} features does not fit one GLWE (N = {N})")
    if a.size != HEADER_WORDS + -(-B // (N // D)) * (k + 1) * N:
        raise ValueError("document block size does not match its document count")
    return {"B": B, "D": D, "P0": int(a[4]), "N": N, "k": k, "glwe": a[HEADER_WORDS:].copy()}


def worst_norm2(cq) -> float:
    """The squared query norm the gadget is planned for, over every query
    (|qq_j| <= 2^(n_e - 1)). The model of params.extprod_var takes the
    rounding errors at the D coefficients a slot sums as independent; under a
    binary key neighbouring coefficients' errors correlate at about 1/2
    (DESIGN.md §8.7), which turns ||W||^2 into (||W||^2 + (sum_j W_j)^2) / 2
    in the dominant term. The plan gets the worst case of that,
    4^(n_e - 1) (sum_j q_w[j]^2 + (sum_j |q_w[j]|)^2) / 2."""
    qw = np.abs(np.asarray(cq.model.q_w, dtype=np.float64))
    return float(4.0 ** (cq.n_e - 1) * 0.5 * (np.sum(qw * qw) + np.sum(qw) ** 2))


def plan_gadget(scheme, cq):
    """(base_log, level) of this model's GGSW queries at scheme.msg_bits, or a
    ValueError that says why there is none."""
    from .params import extprod_plan
    g = extprod_plan(scheme, worst_norm2(cq))
    if g is None:
        raise ValueError(f"both-private search has no GGSW gadget at P0 = {scheme.msg_bits}: the int8 digits stop at "
                         "base_log * level = 49 bits, whose rounding exceeds the 9.2-sigma margin of this width "
                         "(DESIGN.md §8.7); use fewer embedding bits or dimensions")
    return g


class PrivateClient(QueryClient):
    """The key holder: encrypts document blocks and queries, hands out
    evaluation keys, decrypts replies (QueryClient's). Owns the secret context
    of a compiled EncryptedCorpus."""

    def __init__(self, corpus: EncryptedCorpus, count: int = 1024, pack_seed=None, enc_seed: int | None = None):
        """enc_seed: the 64-bit test form of the session's encryption key."""
        from .params import extprod_var
        corpus._need()
        scheme = corpus.scheme.with_msg_bits(corpus.P0)
        self.base_log, self.level = self.gadget = plan_gadget(scheme, corpus.cq)
        # the packing plan sees the leveled step's worst-case variance
        in_var = extprod_var(scheme, worst_norm2(corpus.cq), *self.gadget) / 2.0 ** 128
        super().__init__(corpus, count, in_var, pack_seed)
        self.pack_base_log, self.pack_level = corpus.engine.pack_gadget
        self.base_log, self.level = self.gadget
        self._enc_key = (np.frombuffer(os.urandom(32), np.uint32).copy() if enc_seed is None
                         else corpus.engine.key_from_seed(enc_seed))

    def _ids(self, id0):
        return int.from_bytes(os.urandom(8), "little") if id0 is None else int(id0)

    def encrypt_docs(self, docs, id0: int | None = None) -> np.ndarray:
        """docs f32/f64 [B, D] -> one document block (GLWE g under stream id id0 + g)."""
        import torch
        eng = self.corpus.engine
        docs = np.ascontiguousarray(docs)
        B, D = docs.shape
        eng.set_msg_bits(self.P0)
        dq = eng.quantize(torch.from_numpy(docs).to(eng.device), self.cq.s_e, 0, self.cq.qmin, self.cq.qmax)
        glwe = eng.encrypt_docs_glwe(dq, self._enc_key, self._ids(id0))
        return pack_doc_block(glwe.cpu().numpy().view(np.uint64), B, D, self.P0, eng.params.N, eng.params.k)

    def decrypt_docs(self, block) -> np.ndarray:
        """The quantized documents of a block (the key holder's view; tests)."""
        eng = self.corpus.engine
        bl = unpack_doc_block(block)
        eng.set_msg_bits(self.P0)
        S = bl["N"] // bl["D"]
        G = -(-bl["B"] // S)
        v = eng.decrypt_packed(eng.to_dev(bl["glwe"]), G * bl["N"], 0).cpu().numpy().reshape(G, bl["N"])
        return v[:, :S * bl["D"]].reshape(G * S, bl["D"])[:bl["B"]]

    def encrypt_query(self, q, id0: int | None = None) -> np.ndarray:
        """A reduced query vector -> the GGSW payload sent to the server."""
        eng = self.corpus.engine
        W = self.cq.weights(self.cq.quant(np.asarray(q).reshape(-1)))
        eng.set_msg_bits(self.P0)
        g = eng.encrypt_ggsw(W, self.base_log, self.level, self._enc_key, self._ids(id0))
        return pack_ggsw_query(g.cpu().numpy().view(np.uint64), len(W), self.P0, self.base_log, self.level,
                               eng.params.N, eng.params.k)

    def encrypt_queries(self, vectors, id0: int | None = None) -> list:
        """Q reduced query vectors [Q, D] -> Q GGSW payloads. One random id0;
        query q takes its (k+1) L k mask ids and (k+1) L noise ids from
        id0 + q (k+1) L k on (ggsw_query_ids), so no id repeats under the
        session key."""
        eng = self.corpus.engine
        qq = self.cq.quant(np.atleast_2d(np.asarray(vectors)))
        ids = ggsw_query_ids(self._ids(id0), len(qq), eng.params.k, self.level)
        eng.set_msg_bits(self.P0)
        out = []
        for q, i in zip(qq, ids):
            W = self.cq.weights(q)
            g = eng.encrypt_ggsw(W, self.base_log, self.level, self._enc_key, i)
            out.append(pack_ggsw_query(g.cpu().numpy().view(np.uint64), len(W), self.P0, self.base_log, self.level,
                                       eng.params.N, eng.params.k))
        return out


class PrivateServer(QueryServer):
    """The untrusted host: evaluation keys, the CorpusQuant and P0 only."""

    def __init__(self, eval_keys: dict, cq, P0: int, device: int = 0, scheme=None):
        super().__init__(eval_keys, cq, P0, device, scheme)
        self.base_log, self.level = plan_gadget(self.scheme, cq)

    def _check(self, pl: dict, what: str) -> None:
        if pl["P0"] != self.P0 or pl["N"] != self.scheme.N or pl["k"] != self.scheme.k:
            raise ValueError(f"{what} was encrypted under different parameters")
        if pl["D"] != len(self.cq.model.q_w):
            raise ValueError(f"{what} holds {pl['D']} features, the model {len(self.cq.model.q_w)}")

    def pack_docs(self, block):
        """A document block -> (the device-resident digit operand, B)."""
        bl = unpack_doc_block(block)
        self._check(bl, "document block")
        eng = self.engine
        return eng.pack_docs_glwe(eng.to_dev(bl["glwe"]), bl["B"], bl["D"], self.base_log, self.level), bl["B"]

    def search(self, payload, docs8, B: int, min_similarity: float | None) -> np.ndarray:
        """One GGSW query against B packed encrypted documents -> the reply."""
        eng = self.engine
        pl = unpack_ggsw_query(payload)
        self._check(pl, "query")
        if (pl["base_log"], pl["level"]) != (self.base_log, self.level):
            raise ValueError("query gadget differs from the one the documents were packed for")
        _, cst, T = self.plan(min_similarity)
        ga, gb = eng.search_ggsw(eng.to_dev(pl["ggsw"]), self.base_log, self.level, docs8, int(B), pl["D"], cst, T,
                                 self.bit_levels)
        return pack_reply(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, self.P0, T)

    # -------------------------------------------------- batches of queries --
    def pack_docs_many(self, block):
        """A document block -> (the device-resident operand of search_many, B)."""
        bl = unpack_doc_block(block)
        self._check(bl, "document block")
        eng = self.engine
        return eng.pack_docs_glwe_queries(eng.to_dev(bl["glwe"]), bl["B"], bl["D"], self.base_log,
                                          self.level), bl["B"]

    def search_many(self, payloads, docs, B: int, min_similarity=None) -> list:
        """Q GGSW queries of one key holder against B encrypted documents
        packed by pack_docs_many, in one pass (fhe_search_ggsws_batch) -> a
        LIST of version-2 replies (query.pack_replies), one per chunk of
        query_chunks(Q, B). min_similarity: a float, None, or a sequence of Q
        of them. QueryClient.decrypt_replies takes the list."""
        from .query import pack_replies, query_chunks, thresholds_for
        eng = self.engine
        pls = [unpack_ggsw_query(p) for p in payloads]
        check_ggsw_batch(pls)
        self._check(pls[0], "query 0")
        if (pls[0]["base_log"], pls[0]["level"]) != (self.base_log, self.level):
            raise ValueError("query 0: gadget differs from the one the documents were packed for")
        Q, D = len(pls), pls[0]["D"]
        _, cst, _ = self.plan(None)
        Ts = [self.plan(t)[2] for t in thresholds_for(min_similarity, Q)]
        out = []
        for ch in query_chunks(Q, int(B)):
            g = eng.to_dev(np.concatenate([pls[q]["ggsw"] for q in ch]))
            Tc = [Ts[q] for q in ch]
            ga, gb = eng.search_ggsws(g, self.base_log, self.level, docs, int(B), D, cst, Tc, self.bit_levels)
            out.append(pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, self.P0,
                                    Tc))
        return out


# ------------------------------------------------------ several key holders --
# One evaluation-only host serving tenants that each hold their own keys and
# their own ENCRYPTED documents: every tenant keeps a
# PrivateServer; a call that names several of them runs ONE grouped transposed
# external product and ONE group sign extraction
# (fhe_search_ggsws_group_batch) and answers each tenant in fheicp.query's
# version-2 reply format, word for word what its own
# PrivateServer.search_many returns.
def private_hub_chunks(sizes: dict, cap: int | None = None) -> list:
    """sizes: {name: (Q, B, level)} -> query.hub_chunks's chunks with one more
    rule: a library call has one gadget level (the grouped product's K extent),
    so a tenant whose level differs from the tenant before it starts a new
    chunk. Tenants and queries stay in order; no query is split."""
    from .query import MAX_RESULTS, hub_chunks
    cap = MAX_RESULTS if cap is None else cap
    chunks, run, level = [], {}, None
    for name, (Q, B, lv) in sizes.items():
        if run and int(lv) != level:
            chunks += hub_chunks(run, cap)
            run = {}
        level = int(lv)
        run[name] = (Q, B)
    if run:
        chunks += hub_chunks(run, cap)
    return chunks


class PrivateHub:
    """Tenants with their own keys and their own encrypted documents behind
    one GPU. The host learns which tenant asked, Q and B; documents, queries
    and results stay under each tenant's own key."""

    def __init__(self, device: int = 0):
        self.device = device
        self.tenants = {}       # name -> {"server": PrivateServer, "docs": tensor or None, "B": int}
        self._group = None

    def add_tenant(self, name, eval_keys, cq, P0: int, scheme=None, server=None):
        """Builds the tenant's PrivateServer from its evaluation keys (or
        adopts `server`). Every tenant shares the first one's P0 and scheme
        parameters: ValueError naming the tenant otherwise."""
        if name in self.tenants:
            raise ValueError(f"tenant {name!r} is already registered")
        from .params import params_for_bits
        want = (scheme if scheme is not None else params_for_bits(int(P0))).with_msg_bits(int(P0)) \
            if server is None else server.scheme
        p0 = int(P0) if server is None else int(server.P0)
        for other, rec in self.tenants.items():
            s = rec["server"]
            if int(s.P0) != p0:
                raise ValueError(f"tenant {name!r}: P0 = {p0} differs from tenant {other!r}'s {int(s.P0)}")
            if s.scheme != want:
                raise ValueError(f"tenant {name!r}: scheme parameters differ from tenant {other!r}'s")
            break
        if server is None:
            server = PrivateServer(eval_keys, cq, p0, self.device, scheme)
        self.tenants[name] = {"server": server, "docs": None, "B": 0}
        self.close()
        return server

    def load(self, name, block) -> int:
        """Packs the tenant's document block (pack_docs_many) and keeps the
        operand resident; returns B."""
        rec = self._tenant(name)
        try:
            docs, B = rec["server"].pack_docs_many(block)
        except ValueError as e:
            raise ValueError(f"tenant {name!r}: {e}") from None
        if B < 1:
            raise ValueError(f"tenant {name!r}: an empty document store")
        rec["docs"], rec["B"] = docs, int(B)
        return rec["B"]

    def _tenant(self, name) -> dict:
        if name not in self.tenants:
            raise ValueError(f"unknown tenant {name!r}")
        return self.tenants[name]

    def check_reply(self, name, reply, Q: int) -> dict:
        """A version-2 reply must be the named tenant's: its P0, its loaded
        document count, Q queries and the matching size. ValueError otherwise."""
        from .query import unpack_replies
        rec = self._tenant(name)
        s = rec["server"]
        r = unpack_replies(reply, (s.scheme.k + 1) * s.scheme.N, s.scheme.N)
        if r["P0"] != s.P0 or r["B"] != rec["B"] or r["Q"] != int(Q):
            raise ValueError(f"tenant {name!r}: reply of {r['Q']} queries x {r['B']} documents at P0 = {r['P0']}, "
                             f"expected {int(Q)} x {rec['B']} at P0 = {s.P0}")
        return r

    def group(self):
        if self._group is None:
            from .engine import EngineGroup
            self._group = EngineGroup([rec["server"].engine for rec in self.tenants.values()])
        return self._group

    def close(self) -> None:
        """Releases the group (the tenants' servers stay theirs)."""
        if self._group is not None:
            self._group.close()
            self._group = None

    def _plan(self, requests: dict) -> dict:
        """The per-tenant checks of search_many, before any device work."""
        from .query import thresholds_for
        plan = {}
        for name, (payloads, min_similarity) in requests.items():
            rec = self._tenant(name)
            s = rec["server"]
            if rec["docs"] is None:
                raise ValueError(f"tenant {name!r} has no documents loaded")
            try:
                pls = [unpack_ggsw_query(p) for p in payloads]
                check_ggsw_batch(pls)
                s._check(pls[0], "query 0")
                if (pls[0]["base_log"], pls[0]["level"]) != (s.base_log, s.level):
                    raise ValueError("query 0: gadget differs from the one the documents were packed for")
                ms = thresholds_for(min_similarity, len(pls))
            except ValueError as e:
                raise ValueError(f"tenant {name!r}: {e}") from None
            plan[name] = {"payloads": list(payloads), "pls": pls, "ms": ms, "Ts": [s.plan(t)[2] for t in ms],
                          "cst": s.plan(None)[1]}
        return plan

    def search_many(self, requests: dict) -> dict:
        """requests: {name: (payloads, min_similarity)} -> {name: [replies]},
        version-2 replies for the tenant's QueryClient.decrypt_replies, its
        queries in order. One library call carries at most max(largest B,
        8192) results and one gadget level (private_hub_chunks); a tenant
        alone in a chunk goes through its own PrivateServer.search_many."""
        from .query import pack_replies
        plan = self._plan(requests)
        out = {name: [] for name in requests}
        names = list(self.tenants)
        sizes = {name: (len(plan[name]["pls"]), self.tenants[name]["B"], self.tenants[name]["server"].level)
                 for name in plan}
        for chunk in private_hub_chunks(sizes):
            if len(chunk) == 1:
                name, rng = chunk[0]
                rec, pn = self.tenants[name], plan[name]
                out[name] += rec["server"].search_many([pn["payloads"][q] for q in rng], rec["docs"], rec["B"],
                                                       [pn["ms"][q] for q in rng])
                continue
            items, Tcs = [None] * len(names), {}
            for name, rng in chunk:
                rec, pn = self.tenants[name], plan[name]
                s, pls = rec["server"], pn["pls"]
                g = s.engine.to_dev(np.concatenate([pls[q]["ggsw"] for q in rng]))
                Tcs[name] = [pn["Ts"][q] for q in rng]
                items[names.index(name)] = (g, s.base_log, s.level, rec["docs"], rec["B"], pls[0]["D"], pn["cst"],
                                            Tcs[name], s.bit_levels)
            res = self.group().search_ggsws(items)
            for name, rng in chunk:
                ga, gb = res[names.index(name)]
                rec = self.tenants[name]
                reply = pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), rec["B"],
                                     rec["server"].P0, Tcs[name])
                self.check_reply(name, reply, len(rng))
                out[name].append(reply)
        return out
