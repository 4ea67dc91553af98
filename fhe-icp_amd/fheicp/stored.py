"""Stored-ciphertext search with two parties.

The stored-ciphertext mode (fheicp.corpus: documents kept as seeded LWEs and
searched without decryption) with its two roles in two contexts:

  * CorpusClient, the key holder: encrypts documents (EncryptedCorpus's
    encrypt_docs / payloads), hands out evaluation keys with a packing key and
    decrypts replies;
  * CorpusServer, the host: holds evaluation keys, the public mask key, the
    CorpusQuant and P0 only. It keeps a client's encrypted documents resident
    and scores Q CLEAR queries against them in one pass per chunk
    (fhe_search_seeded_queries_batch), answering with packed GLWEs that only
    the client can open.

The host sees the queries, the thresholds, Q, B and D; it never sees a
document, a score or a threshold bit. Replies are the version-2 format of
fheicp.query (pack_replies / unpack_replies) unchanged; the width field
carries the chunk's own width P <= P0 (EncryptedCorpus.plan_many).
"""
from __future__ import annotations

import numpy as np

from .corpus import CorpusQuant, EncryptedCorpus
from .query import load_eval_keys, pack_replies, query_chunks, thresholds_for, unpack_replies


def leveled_in_var(cq: CorpusQuant, P0: int, scheme) -> float:
    """Worst-case variance (torus units) of a leveled accumulator of this mode.

    plan_many's rescaled weights satisfy sum_j |Wr_j| (2^n_e - 1) < 2^(P0 - 1)
    (acc - T spans at most P bits and the row carries 2^(P0 - P)), so
    ||Wr||_2 <= ||Wr||_1 < 2^(P0 - 1) / (2^n_e - 1), with equality approached
    by a query concentrated on one feature: up to sqrt(D) times the
    all-features case. Each stored LWE carries fresh TUniform(glwe_noise_bits)
    noise, so the accumulator's variance is at most that bound squared times
    the fresh variance."""
    from .params import _tuniform_var
    bound = 2.0 ** (int(P0) - 1) / float(2 ** int(cq.n_e) - 1)
    return bound * bound * _tuniform_var(scheme.glwe_noise_bits) / 2.0 ** 128


def parse_replies(replies, P0: int, glwe_words: int | None = None, N: int | None = None) -> list:
    """The list CorpusServer.search_many returns (or one version-2 reply) ->
    unpacked replies, each with a width in [4, P0] (its "P0" field is the
    chunk's width P). No device needed."""
    if isinstance(replies, np.ndarray):
        replies = [replies]
    out = []
    for i, reply in enumerate(replies):
        r = unpack_replies(reply, glwe_words, N)
        if not 4 <= r["P0"] <= int(P0):
            raise ValueError(f"reply {i} was computed at width {r['P0']}, outside [4, {int(P0)}]")
        out.append(r)
    return out


class CorpusClient:
    """The key holder of the stored-ciphertext mode: owns the secret context of
    a compiled EncryptedCorpus."""

    def __init__(self, corpus: EncryptedCorpus, count: int = 1024, in_var: float | None = None, pack_seed=None):
        """Generates the packing key planned once at P0 (at P < P0 the margin
        2^(63 - P) / sigma only grows) for replies of up to `count` results per
        GLWE. in_var defaults to leveled_in_var, the l1 bound of this mode's
        weights (pack_seed: the 64-bit test form)."""
        from .params import pack_plan, pack_sigmas
        corpus._need()
        self.corpus = corpus
        self.cq, self.P0 = corpus.cq, corpus.P0
        scheme = corpus.scheme.with_msg_bits(self.P0)
        self.in_var = leveled_in_var(self.cq, self.P0, scheme) if in_var is None else float(in_var)
        self.base_log, self.level, self.bit_levels = pack_plan(scheme, count, self.in_var)
        #: the plan's margin in sigmas (below 9.2 when no gadget reaches the bar)
        self.margin = pack_sigmas(scheme, count, self.in_var, self.base_log, self.level, 63 - self.P0)
        corpus.engine.keygen_pack(self.base_log, self.level, seed=pack_seed)

    def encrypt_docs(self, docs, id0=None):
        return self.corpus.encrypt_docs(docs, id0)

    def payloads(self, bodies, ids):
        return self.corpus.payloads(bodies, ids)

    def eval_keys(self) -> dict:
        """What the host gets: bsk, ksk, the gadgets' keys, the packing key
        with its gadget and the bit prefix. No secret key."""
        d = self.corpus.engine.export_eval_keys()
        d["pack_bit_levels"] = np.array([self.bit_levels], dtype=np.int64)
        return d

    def decrypt_replies(self, replies):
        """-> (acc int64 [Q, B], below int64 [Q, B]) device tensors, the
        chunks' queries in order. Each reply is decrypted at its own width and
        T_q is added back per query."""
        import torch
        eng = self.corpus.engine
        n1 = (eng.params.k + 1) * eng.params.N
        accs, belows = [], []
        for r in parse_replies(replies, self.P0, n1, eng.params.N):
            Q, B = r["Q"], r["B"]
            eng.set_msg_bits(r["P0"])
            T = eng.to_dev(np.array(r["T"], dtype=np.int64)).reshape(Q, 1)
            accs.append(eng.decrypt_packed(eng.to_dev(r["glwe_acc"]), Q * B, 0).reshape(Q, B) + T)
            belows.append(eng.decrypt_packed(eng.to_dev(r["glwe_bit"]), Q * B, 1).reshape(Q, B))
        if not accs:
            raise ValueError("no replies to decrypt")
        return torch.cat(accs), torch.cat(belows)

    def top_k(self, acc, below, k: int, base_idx: int = 0):
        return self.corpus.engine.topk(acc, below, k, base_idx)


class CorpusServer:
    """The host: evaluation keys, the public mask key, the CorpusQuant and P0
    only. Honest-but-curious: it runs the search as written."""

    def __init__(self, eval_keys: dict, cq: CorpusQuant, P0: int, mask_key, device: int = 0, scheme=None):
        from .engine import Engine
        if "pack_key" not in eval_keys:
            raise ValueError("the evaluation keys hold no packing key")
        self.cq, self.P0 = cq, int(P0)
        self._plan = EncryptedCorpus(cq, scheme)  # planning only: never compiled, holds no key
        if self._plan.P0 != self.P0:
            raise ValueError(f"P0 = {self.P0} does not match the model's worst-case width {self._plan.P0}")
        self.scheme = self._plan.scheme
        self.mask_key = np.ascontiguousarray(mask_key, dtype=np.uint32).reshape(8).copy()
        self.engine = Engine(self.scheme, device)
        self.engine.import_eval_keys(eval_keys)
        self.bit_levels = int(np.asarray(eval_keys.get("pack_bit_levels", [0])).reshape(-1)[0])
        self.body = self.ids = None

    @classmethod
    def from_npz(cls, path: str, cq: CorpusQuant, P0: int, mask_key, device: int = 0, scheme=None) -> "CorpusServer":
        return cls(load_eval_keys(path), cq, P0, mask_key, device, scheme)

    def load(self, bodies, ids) -> int:
        """Make a corpus resident: bodies uint64 [B, D], ids uint64 [B]."""
        bodies = np.ascontiguousarray(bodies, dtype=np.uint64)
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if bodies.ndim != 2 or bodies.shape[0] != ids.size or bodies.shape[0] < 1:
            raise ValueError("load needs bodies [B, D] and B stream ids, B >= 1")
        if bodies.shape[1] != len(self.cq.model.q_w):
            raise ValueError(f"documents hold {bodies.shape[1]} features, the model {len(self.cq.model.q_w)}")
        self.body, self.ids = self.engine.to_dev(bodies), self.engine.to_dev(ids)
        return int(ids.size)

    def search_many(self, queries, min_similarity=None) -> list:
        """Q clear queries against the resident corpus -> a LIST of version-2
        replies, one per chunk of query_chunks(Q, B), each planned on its own
        (its width field is the chunk's P). min_similarity: a float, None, or
        Q of them. CorpusClient.decrypt_replies takes the list."""
        if self.body is None:
            raise RuntimeError("no resident corpus: call load() first")
        eng = self.engine
        queries = np.atleast_2d(np.asarray(queries))
        Q, B = queries.shape[0], int(self.body.shape[0])
        ts = thresholds_for(min_similarity, Q)
        out = []
        for ch in query_chunks(Q, B):
            Wr, cst, Ts, P = self._plan.plan_many(queries[ch.start:ch.stop], [ts[q] for q in ch])
            eng.set_msg_bits(P)
            ga, gb = eng.search_seeded_queries(self.body, self.ids, self.mask_key, eng.to_dev(Wr), cst, Ts,
                                               self.bit_levels)
            out.append(pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, P, Ts))
        return out

    def search(self, query, min_similarity=None) -> np.ndarray:
        """One query: the single reply of search_many([query])."""
        return self.search_many(np.asarray(query).reshape(1, -1), min_similarity)[0]
