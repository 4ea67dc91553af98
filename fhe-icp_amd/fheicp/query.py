"""Private-query search: an encrypted query against a clear document store.

The third deployment shape. The reference's store holds
plaintext embeddings (``EncryptedDocument.encrypted_embedding`` is the PCA
vector, batch_operations.py:175-178); here the documents stay as they are and
the QUERY is what arrives encrypted:

  * the client quantizes its query with the corpus quantizer,
    ``qq = E.quant(q)`` (fheicp.corpus.CorpusQuant), and encrypts the D values
    as seeded LWEs at the worst-case width P0 (fhe_encrypt_seeded_batch, one
    row): D body words, a 64-bit stream id and the public mask key;
  * the server quantizes its documents the same way, ``dq = E.quant(d)``,
    packs them once for the i8 matrix cores (fhe_query_docs_pack) and computes
    ``acc_b = sum_j q_w[j] * qq_j * dq[b, j] + q_b'`` homomorphically
    (fhe_compare_query_batch: the query's byte planes, one integer GEMM, sign
    extraction of ``acc - T``).

It is the bilinear quantisation of fheicp.corpus with the roles swapped, so
the expected values are the same restatement (oracle/quant_ref.py,
``corpus_*``). The server never sees the query, so every compare runs at P0
(no per-query width, no rescale shift) and the threshold is placed on the
worst-case range [-bound, bound].

Query payload (uint64 vector):
    [MAGIC, 1, D, P0, id0, mask key (4 words), k*N, body_0 .. body_{D-1}]

Several queries of one key holder against the same documents go through in
one pass: encrypt_queries, compare_many, and for two parties
QueryServer.search_many / QueryClient.decrypt_replies. A batch is a list of
the payloads above whose stream-id ranges [id0, id0 + D) are disjoint.
"""
from __future__ import annotations

import os

import numpy as np

from .corpus import HEADER_WORDS, EncryptedCorpus

QUERY_VERSION = "fheicp-seeded-query-v1"
MAGIC = int.from_bytes(b"FHEICPQY", "little")


def pack_query(body, id0: int, P0: int, mask_key, big: int) -> np.ndarray:
    body = np.asarray(body, dtype=np.uint64).reshape(-1)
    mk = np.ascontiguousarray(mask_key, dtype=np.uint32).view(np.uint64)
    head = np.array([MAGIC, 1, body.size, P0, np.uint64(id0)], dtype=np.uint64)
    return np.concatenate([head, mk, np.array([big], np.uint64), body])


def unpack_query(arr) -> dict:
    a = np.asarray(arr)
    if a.dtype != np.uint64 or a.ndim != 1 or a.size < HEADER_WORDS or int(a[0]) != MAGIC:
        raise ValueError("not an fheicp seeded-query payload")
    if int(a[1]) != 1:
        raise ValueError(f"unsupported query payload version {int(a[1])}")
    D = int(a[2])
    if a.size != HEADER_WORDS + D:
        raise ValueError(f"query payload holds {a.size - HEADER_WORDS} bodies, header says {D}")
    return {"D": D, "P0": int(a[3]), "id0": int(a[4]), "mask_key": a[5:9].copy().view(np.uint32),
            "big": int(a[9]), "body": a[HEADER_WORDS:].copy()}


# ------------------------------------------------------ batches of queries --
# Several queries of one key holder answered in one pass: a
# batch is a list of the payloads above, no new format.
MAX_RESULTS = 8192  # results (Q * B) one library call carries, unless B alone is larger


def check_query_batch(pls) -> None:
    """The unpacked payloads of one batch agree in P0, big, D and mask key,
    and no two stream-id ranges [id0, id0 + D) overlap modulo 2^64 (an id must
    not repeat under one mask key). ValueError names the offending query."""
    if not pls:
        raise ValueError("an empty batch of queries")
    first = pls[0]
    for i, pl in enumerate(pls[1:], 1):
        for field, what in (("P0", "width P0"), ("big", "ciphertext size"), ("D", "dimension D")):
            if pl[field] != first[field]:
                raise ValueError(f"query {i}: {what} {pl[field]} differs from query 0's {first[field]}")
        if not np.array_equal(pl["mask_key"], first["mask_key"]):
            raise ValueError(f"query {i}: mask key differs from query 0's")
    D = int(first["D"])
    order = sorted(range(len(pls)), key=lambda i: int(pls[i]["id0"]))
    for a, b in zip(order, order[1:] + order[:1]):
        if a == b:
            break  # one query: its D <= 65536 ids cannot meet themselves
        if (int(pls[b]["id0"]) - int(pls[a]["id0"])) % (1 << 64) < D:
            raise ValueError(f"query {max(a, b)}: stream ids [id0, id0 + {D}) overlap query {min(a, b)}'s")


def query_chunks(Q: int, B: int, cap: int = MAX_RESULTS) -> list:
    """range(Q) split into consecutive ranges of max(1, cap // B) queries: one
    library call carries at most max(B, cap) results."""
    if Q < 0 or B < 1 or cap < 1:
        raise ValueError("query_chunks needs Q >= 0, B >= 1, cap >= 1")
    step = max(1, cap // B)
    return [range(s, min(Q, s + step)) for s in range(0, Q, step)]


def thresholds_for(min_similarity, Q: int) -> list:
    """A float, None, or a sequence of Q of them -> a list of Q."""
    if min_similarity is None or np.isscalar(min_similarity):
        return [min_similarity] * Q
    ts = list(min_similarity)
    if len(ts) != Q:
        raise ValueError(f"{len(ts)} thresholds for {Q} queries")
    return ts


class EncryptedQuerySearch:
    """Both sides of the private-query mode over one EncryptedCorpus: its
    context, keys, mask key, noise key, CorpusQuant and P0 (so
    persist.save_corpus / load_corpus carry everything this mode needs)."""

    MAX_BITS = 8  # the documents are the GEMM's i8 operand

    def __init__(self, corpus: EncryptedCorpus):
        self.corpus = corpus
        self.cq = corpus.cq
        self.P0 = corpus.P0

    # ----------------------------------------------------------- planning --
    def bound(self) -> int:
        """max |acc| over every query and document: the value behind worst_msg_bits."""
        qw = np.abs(np.asarray(self.cq.model.q_w, dtype=np.int64))
        return int(qw.sum()) * 4 ** (self.cq.n_e - 1) + abs(self.cq.q_b)

    def plan(self, min_similarity: float | None):
        """Clear per-search constants (w int64 [D], cst, T). The server cannot
        see the query: T sits on the worst-case range, w = q_w."""
        b = self.bound()
        T = self.cq.threshold_int(-b, b, min_similarity) if min_similarity is not None else -b
        return np.asarray(self.cq.model.q_w, dtype=np.int64).copy(), self.cq.q_b, T

    def check(self, pl: dict) -> None:
        c = self.corpus
        if pl["P0"] != self.P0 or pl["big"] != c.scheme.k * c.scheme.N:
            raise ValueError("query was encrypted under different parameters")
        if c.mask_key is not None and not np.array_equal(pl["mask_key"], c.mask_key):
            raise ValueError("query was encrypted under a different mask key")
        if pl["D"] != len(self.cq.model.q_w):
            raise ValueError(f"query holds {pl['D']} features, the model {len(self.cq.model.q_w)}")

    # ------------------------------------------------------------- client --
    def encrypt_query(self, q, id0: int | None = None) -> np.ndarray:
        """A reduced query vector -> the uint64 payload sent to the server."""
        c = self.corpus
        c._need()
        eng = c.engine
        qq = self.cq.quant(np.asarray(q).reshape(1, -1))
        if id0 is None:
            id0 = int.from_bytes(os.urandom(8), "little")
        eng.set_msg_bits(self.P0)
        ids = eng.to_dev(np.array([id0], dtype=np.uint64))
        body = eng.encrypt_seeded(eng.to_dev(qq), c.mask_key, c._noise_key, ids)
        return pack_query(body.cpu().numpy().view(np.uint64)[0], id0, self.P0, c.mask_key, c.scheme.k * c.scheme.N)

    def decrypt_query(self, payload) -> np.ndarray:
        """The quantized query (the key holder's view; tests)."""
        c = self.corpus
        c._need()
        pl = unpack_query(payload)
        self.check(pl)
        return c.decrypt_docs(pl["body"][None, :], [pl["id0"]])[0]

    # ------------------------------------------------------------- server --
    def pack_docs(self, docs):
        """docs f32/f64 [B, D] (host array or device tensor) -> the packed,
        device-resident i8 corpus (a uint8 tensor; keep B beside it)."""
        import torch
        if self.cq.n_e > self.MAX_BITS:
            raise ValueError(f"private-query search needs embedding bits n_e <= {self.MAX_BITS}, got {self.cq.n_e} "
                             "(the documents are the i8 operand of the matrix cores)")
        self.corpus._need()
        eng = self.corpus.engine
        dd = docs if isinstance(docs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(docs))
        dq = eng.quantize(dd.to(eng.device).contiguous(), self.cq.s_e, 0, self.cq.qmin, self.cq.qmax)
        return eng.pack_docs(dq)

    def compare(self, payload, docs8, B: int, min_similarity: float | None):
        """-> (acc int64 [B], below int64 [B]) device tensors."""
        self.corpus._need()
        eng = self.corpus.engine
        pl = unpack_query(payload)
        self.check(pl)
        w, cst, T = self.plan(min_similarity)
        eng.set_msg_bits(self.P0)
        return eng.compare_query(eng.to_dev(pl["body"]), pl["id0"], pl["mask_key"], docs8, int(B), pl["D"],
                                 eng.to_dev(w), cst, T)

    def scores(self, acc) -> np.ndarray:
        return self.corpus.scores(acc)

    # -------------------------------------------------- batches of queries --
    def encrypt_queries(self, vectors, id0: int | None = None) -> list:
        """Q reduced query vectors [Q, D] -> Q payloads in one encryption
        call. Query q takes the stream ids [id0 + q D, id0 + (q + 1) D)
        modulo 2^64 from a fresh random id0: disjoint within the batch."""
        c = self.corpus
        c._need()
        eng = c.engine
        qq = self.cq.quant(np.atleast_2d(np.asarray(vectors)))
        Q, D = qq.shape
        if id0 is None:
            id0 = int.from_bytes(os.urandom(8), "little")
        ids = [(int(id0) + q * D) % (1 << 64) for q in range(Q)]
        eng.set_msg_bits(self.P0)
        body = eng.encrypt_seeded(eng.to_dev(qq), c.mask_key, c._noise_key, eng.to_dev(np.array(ids, dtype=np.uint64)))
        body = body.cpu().numpy().view(np.uint64)
        return [pack_query(body[q], ids[q], self.P0, c.mask_key, c.scheme.k * c.scheme.N) for q in range(Q)]

    def plan_many(self, min_similarity, Q: int):
        """(w, cst, [T_0 .. T_{Q-1}]): plan() per query threshold."""
        w, cst, _ = self.plan(None)
        return w, cst, [self.plan(t)[2] for t in thresholds_for(min_similarity, Q)]

    def compare_many(self, payloads, docs8, B: int, min_similarity=None):
        """Q payloads of this key holder against the same packed documents
        in one pass per chunk of query_chunks(Q, B) (fhe_compare_queries_batch)
        -> (acc int64 [Q, B], below int64 [Q, B]) device tensors.
        min_similarity: a float, None, or a sequence of Q of them."""
        import torch
        self.corpus._need()
        eng = self.corpus.engine
        pls = [unpack_query(p) for p in payloads]
        check_query_batch(pls)
        self.check(pls[0])
        Q, D = len(pls), pls[0]["D"]
        w, cst, Ts = self.plan_many(min_similarity, Q)
        eng.set_msg_bits(self.P0)
        wd = eng.to_dev(w)
        accs, belows = [], []
        for ch in query_chunks(Q, int(B)):
            body = eng.to_dev(np.stack([pls[q]["body"] for q in ch]))
            ids = eng.to_dev(np.array([pls[q]["id0"] for q in ch], dtype=np.uint64))
            acc, below = eng.compare_queries(body, ids, pls[0]["mask_key"], docs8, int(B), D, wd, cst,
                                             [Ts[q] for q in ch])
            accs.append(acc)
            belows.append(below)
        return torch.cat(accs), torch.cat(belows)


# ------------------------------------------------------------- two parties --
# The same search with the two roles in two contexts: the
# client keeps the secret key; the server holds evaluation keys only and
# answers with packed GLWEs.
#
# Reply (uint64 vector):
#     [REPLY_MAGIC, version | P0 << 32, B, T (two's complement),
#      GLWEs of acc - T: ceil(B / N) x (k+1)N words, GLWEs of [acc < T]: the same]
REPLY_MAGIC = int.from_bytes(b"FHEICPRP", "little")
REPLY_HEADER_WORDS = 4
# variance (torus units) of the leveled accumulator the plan assumes: the
# worst-case leveled sigma of DESIGN.md §8, 2^-33
LEVELED_VAR = (2.0 ** -33) ** 2


def pack_reply(glwe_acc, glwe_bit, B: int, P0: int, T: int) -> np.ndarray:
    ga = np.asarray(glwe_acc, dtype=np.uint64).reshape(-1)
    gb = np.asarray(glwe_bit, dtype=np.uint64).reshape(-1)
    head = np.array([REPLY_MAGIC, 1 | (int(P0) << 32), int(B), int(T) % (1 << 64)], dtype=np.uint64)
    return np.concatenate([head, ga, gb])


def unpack_reply(arr) -> dict:
    a = np.asarray(arr)
    if a.dtype != np.uint64 or a.ndim != 1 or a.size < REPLY_HEADER_WORDS or int(a[0]) != REPLY_MAGIC:
        raise ValueError("not an fheicp packed reply")
    if int(a[1]) & 0xFFFFFFFF != 1:
        raise ValueError(f"unsupported reply version {int(a[1]) & 0xFFFFFFFF}")
    words = a.size - REPLY_HEADER_WORDS
    if words % 2:
        raise ValueError("reply holds an odd number of GLWE words")
    T = int(a[3])
    return {"P0": int(a[1]) >> 32, "B": int(a[2]), "T": T - (1 << 64) if T >> 63 else T,
            "glwe_acc": a[REPLY_HEADER_WORDS:REPLY_HEADER_WORDS + words // 2].copy(),
            "glwe_bit": a[REPLY_HEADER_WORDS + words // 2:].copy()}


# Reply to a batch of queries, version 2 (uint64 vector):
#     [REPLY_MAGIC, 2 | P0 << 32, B, Q, T_0 .. T_{Q-1} (two's complement),
#      GLWEs of acc - T_q: ceil(Q B / N) x (k+1)N words, GLWEs of the bits: the same]
# Result (q, b) is coefficient (q B + b) mod N of GLWE (q B + b) / N.
def pack_replies(glwe_acc, glwe_bit, B: int, P0: int, Ts) -> np.ndarray:
    ga = np.asarray(glwe_acc, dtype=np.uint64).reshape(-1)
    gb = np.asarray(glwe_bit, dtype=np.uint64).reshape(-1)
    head = np.array([REPLY_MAGIC, 2 | (int(P0) << 32), int(B), len(Ts)] + [int(T) % (1 << 64) for T in Ts],
                    dtype=np.uint64)
    return np.concatenate([head, ga, gb])


def unpack_replies(arr, glwe_words: int | None = None, N: int | None = None) -> dict:
    """A version-2 reply. With glwe_words = (k+1)N and N it also rejects a
    size that does not match ceil(Q B / N) GLWEs per block."""
    a = np.asarray(arr)
    if a.dtype != np.uint64 or a.ndim != 1 or a.size < REPLY_HEADER_WORDS or int(a[0]) != REPLY_MAGIC:
        raise ValueError("not an fheicp packed reply")
    if int(a[1]) & 0xFFFFFFFF != 2:
        raise ValueError(f"unsupported batched reply version {int(a[1]) & 0xFFFFFFFF}")
    B, Q = int(a[2]), int(a[3])
    if B < 1 or Q < 1 or a.size < REPLY_HEADER_WORDS + Q:
        raise ValueError(f"reply header names {Q} queries of {B} documents in {a.size} words")
    words = a.size - REPLY_HEADER_WORDS - Q
    if words % 2:
        raise ValueError("reply holds an odd number of GLWE words")
    if glwe_words is not None and words // 2 != -(-(Q * B) // int(N)) * int(glwe_words):
        raise ValueError(f"reply size does not match {Q} queries of {B} documents")
    Ts = [int(t) - (1 << 64) if int(t) >> 63 else int(t) for t in a[REPLY_HEADER_WORDS:REPLY_HEADER_WORDS + Q]]
    g0 = REPLY_HEADER_WORDS + Q
    return {"P0": int(a[1]) >> 32, "B": B, "Q": Q, "T": Ts, "glwe_acc": a[g0:g0 + words // 2].copy(),
            "glwe_bit": a[g0 + words // 2:].copy()}


def save_eval_keys(path: str, keys: dict) -> None:
    """Evaluation keys (QueryClient.eval_keys) -> one .npz of plain arrays."""
    with open(path, "wb") as f:
        np.savez(f, **{k: np.asarray(v) for k, v in keys.items()})


def load_eval_keys(path: str) -> dict:
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


class QueryClient:
    """The key holder: encrypts queries, hands out evaluation keys, decrypts
    replies. Owns the secret context of a compiled EncryptedCorpus."""

    def __init__(self, corpus: EncryptedCorpus, count: int = 1024, in_var: float = LEVELED_VAR, pack_seed=None):
        """Generates the packing key planned for replies of up to `count`
        results per GLWE (params.pack_plan; pack_seed: the 64-bit test form)."""
        from .params import pack_plan, pack_sigmas
        corpus._need()
        self.corpus = corpus
        self.single = EncryptedQuerySearch(corpus)
        self.cq, self.P0 = corpus.cq, corpus.P0
        scheme = corpus.scheme.with_msg_bits(self.P0)
        self.base_log, self.level, self.bit_levels = pack_plan(scheme, count, in_var)
        #: the plan's margin in sigmas (below 9.2 when no gadget reaches the bar)
        self.margin = pack_sigmas(scheme, count, in_var, self.base_log, self.level, 63 - self.P0)
        corpus.engine.keygen_pack(self.base_log, self.level, seed=pack_seed,
                                  mask_key=corpus.next_key_mask() if corpus.seeded_keys else None)

    def encrypt_query(self, q, id0: int | None = None) -> np.ndarray:
        return self.single.encrypt_query(q, id0)

    def eval_keys(self, seeded: bool | None = None) -> dict:
        """What the server gets: bsk, ksk, the gadgets' keys, the packing key
        with its gadget and the bit prefix. No secret key. On a corpus compiled
        with seeded_keys the dict is the seeded form (§8.16: bodies and mask
        keys); eval_keys(seeded=False) is the full form of the same keys."""
        d = self.corpus.engine.export_eval_keys(seeded=self.corpus.seeded_keys if seeded is None else seeded)
        d["pack_bit_levels"] = np.array([self.bit_levels], dtype=np.int64)
        return d

    def decrypt_reply(self, reply):
        """-> (acc int64 [B], below int64 [B]) device tensors."""
        eng = self.corpus.engine
        r = unpack_reply(reply)
        if r["P0"] != self.P0:
            raise ValueError("reply was computed at a different width")
        n1 = (eng.params.k + 1) * eng.params.N
        if r["glwe_acc"].size != eng.glwe_count(r["B"]) * n1:
            raise ValueError("reply size does not match its document count")
        eng.set_msg_bits(self.P0)
        acc = eng.decrypt_packed(eng.to_dev(r["glwe_acc"]), r["B"], 0) + r["T"]
        below = eng.decrypt_packed(eng.to_dev(r["glwe_bit"]), r["B"], 1)
        return acc, below

    def encrypt_queries(self, vectors, id0: int | None = None) -> list:
        """[Q, D] query vectors -> Q payloads with fresh, disjoint stream ids."""
        return self.single.encrypt_queries(vectors, id0)

    def decrypt_replies(self, replies):
        """The list QueryServer.search_many returns (or one version-2 reply)
        -> (acc int64 [Q, B], below int64 [Q, B]) device tensors, the chunks'
        queries in order. Adds T_q back per query."""
        import torch
        eng = self.corpus.engine
        if isinstance(replies, np.ndarray):
            replies = [replies]
        n1 = (eng.params.k + 1) * eng.params.N
        eng.set_msg_bits(self.P0)
        accs, belows = [], []
        for reply in replies:
            r = unpack_replies(reply, n1, eng.params.N)
            if r["P0"] != self.P0:
                raise ValueError("reply was computed at a different width")
            Q, B = r["Q"], r["B"]
            T = eng.to_dev(np.array(r["T"], dtype=np.int64)).reshape(Q, 1)
            accs.append(eng.decrypt_packed(eng.to_dev(r["glwe_acc"]), Q * B, 0).reshape(Q, B) + T)
            belows.append(eng.decrypt_packed(eng.to_dev(r["glwe_bit"]), Q * B, 1).reshape(Q, B))
        return torch.cat(accs), torch.cat(belows)

    def top_k(self, acc, below, k: int, base_idx: int = 0):
        return self.corpus.engine.topk(acc, below, k, base_idx)


class QueryServer:
    """The document holder: evaluation keys, the CorpusQuant and P0 only."""

    MAX_BITS = EncryptedQuerySearch.MAX_BITS

    def __init__(self, eval_keys: dict, cq, P0: int, device: int = 0, scheme=None):
        from .engine import Engine
        from .params import params_for_bits
        if "pack_key" not in eval_keys and "pack_key_body" not in eval_keys:
            raise ValueError("the evaluation keys hold no packing key")
        self.cq, self.P0 = cq, int(P0)
        self.scheme = (scheme if scheme is not None else params_for_bits(self.P0)).with_msg_bits(self.P0)
        self.engine = Engine(self.scheme, device)
        self.engine.import_eval_keys(eval_keys)
        self.bit_levels = int(np.asarray(eval_keys.get("pack_bit_levels", [0])).reshape(-1)[0])

    @classmethod
    def from_npz(cls, path: str, cq, P0: int, device: int = 0, scheme=None) -> "QueryServer":
        return cls(load_eval_keys(path), cq, P0, device, scheme)

    def bound(self) -> int:
        qw = np.abs(np.asarray(self.cq.model.q_w, dtype=np.int64))
        return int(qw.sum()) * 4 ** (self.cq.n_e - 1) + abs(self.cq.q_b)

    def plan(self, min_similarity: float | None):
        """(w, cst, T) as EncryptedQuerySearch.plan: T on the worst-case range."""
        b = self.bound()
        T = self.cq.threshold_int(-b, b, min_similarity) if min_similarity is not None else -b
        return np.asarray(self.cq.model.q_w, dtype=np.int64).copy(), self.cq.q_b, T

    def pack_docs(self, docs):
        import torch
        if self.cq.n_e > self.MAX_BITS:
            raise ValueError(f"private-query search needs embedding bits n_e <= {self.MAX_BITS}, got {self.cq.n_e}")
        eng = self.engine
        dd = docs if isinstance(docs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(docs))
        dq = eng.quantize(dd.to(eng.device).contiguous(), self.cq.s_e, 0, self.cq.qmin, self.cq.qmax)
        return eng.pack_docs(dq)

    def search(self, payload, docs8, B: int, min_similarity: float | None) -> np.ndarray:
        """One encrypted query against B packed documents -> the reply."""
        eng = self.engine
        pl = unpack_query(payload)
        if pl["P0"] != self.P0 or pl["big"] != self.scheme.k * self.scheme.N:
            raise ValueError("query was encrypted under different parameters")
        if pl["D"] != len(self.cq.model.q_w):
            raise ValueError(f"query holds {pl['D']} features, the model {len(self.cq.model.q_w)}")
        w, cst, T = self.plan(min_similarity)
        ga, gb = eng.search_query(eng.to_dev(pl["body"]), pl["id0"], pl["mask_key"], docs8, int(B), pl["D"],
                                  eng.to_dev(w), cst, T, self.bit_levels)
        return pack_reply(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, self.P0, T)

    def search_many(self, payloads, docs8, B: int, min_similarity=None) -> list:
        """Q encrypted queries of one key holder against B packed documents
        in one pass (fhe_search_queries_batch) -> a LIST of version-2 replies,
        always: one per chunk of query_chunks(Q, B), so a single element
        unless Q * B exceeds max(B, 8192) results. min_similarity: a float,
        None, or a sequence of Q of them. QueryClient.decrypt_replies takes
        the list."""
        eng = self.engine
        pls = [unpack_query(p) for p in payloads]
        check_query_batch(pls)
        pl = pls[0]
        if pl["P0"] != self.P0 or pl["big"] != self.scheme.k * self.scheme.N:
            raise ValueError("query 0 was encrypted under different parameters")
        if pl["D"] != len(self.cq.model.q_w):
            raise ValueError(f"query 0 holds {pl['D']} features, the model {len(self.cq.model.q_w)}")
        Q = len(pls)
        w, cst, _ = self.plan(None)
        Ts = [self.plan(t)[2] for t in thresholds_for(min_similarity, Q)]
        wd = eng.to_dev(w)
        out = []
        for ch in query_chunks(Q, int(B)):
            body = eng.to_dev(np.stack([pls[q]["body"] for q in ch]))
            ids = eng.to_dev(np.array([pls[q]["id0"] for q in ch], dtype=np.uint64))
            Tc = [Ts[q] for q in ch]
            ga, gb = eng.search_queries(body, ids, pl["mask_key"], docs8, int(B), pl["D"], wd, cst, Tc,
                                        self.bit_levels)
            out.append(pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, self.P0,
                                    Tc))
        return out


# ------------------------------------------------------ several key holders --
# One evaluation-only host serving tenants that each hold their own keys and
# their own documents: every tenant keeps a QueryServer; a
# call that names several of them runs their sign extractions in one group
# launch sequence (fhe_search_query_group_batch) and answers each tenant in
# the version-2 reply format above, word for word what its own
# QueryServer.search_many returns.
def hub_chunks(sizes: dict, cap: int = MAX_RESULTS) -> list:
    """sizes: {name: (Q, B)} -> a list of chunks, each a list of (name,
    range of that tenant's queries), tenants and queries in order. A chunk
    carries at most max(cap, the largest B) results: a query's B results are
    never split, and a tenant's piece is as many whole queries as still fit."""
    if cap < 1:
        raise ValueError("hub_chunks needs cap >= 1")
    chunks, cur, used = [], [], 0
    for name, (Q, B) in sizes.items():
        Q, B = int(Q), int(B)
        if Q < 0 or B < 1:
            raise ValueError(f"tenant {name!r}: hub_chunks needs Q >= 0 and B >= 1")
        q = 0
        while q < Q:
            fit = max(0, cap - used) // B
            if fit == 0 and cur:          # no room left for one more query: close the chunk
                chunks.append(cur)
                cur, used = [], 0
                continue
            take = min(Q - q, max(fit, 1))  # an empty chunk takes one query even when B > cap
            cur.append((name, range(q, q + take)))
            used += take * B
            q += take
    if cur:
        chunks.append(cur)
    return chunks


class QueryHub:
    """Tenants with their own keys and documents behind one GPU. The host
    learns which tenant asked; each tenant's values stay under its own key."""

    def __init__(self, device: int = 0):
        self.device = device
        self.tenants = {}       # name -> {"server": QueryServer, "docs8": tensor or None, "B": int}
        self._group = None

    def add_tenant(self, name, eval_keys, cq, P0: int, scheme=None, server=None):
        """Builds the tenant's QueryServer from its evaluation keys (or adopts
        `server`). Every tenant shares the first one's P0 and scheme
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
            server = QueryServer(eval_keys, cq, p0, self.device, scheme)
        self.tenants[name] = {"server": server, "docs8": None, "B": 0}
        self._group = None
        return server

    def load(self, name, docs) -> int:
        """Packs the tenant's documents and keeps them resident; returns B."""
        rec = self._tenant(name)
        B = int(docs.shape[0])
        if B < 1:
            raise ValueError(f"tenant {name!r}: an empty document store")
        rec["docs8"], rec["B"] = rec["server"].pack_docs(docs), B
        return B

    def _tenant(self, name) -> dict:
        if name not in self.tenants:
            raise ValueError(f"unknown tenant {name!r}")
        return self.tenants[name]

    def check_reply(self, name, reply, Q: int) -> dict:
        """A version-2 reply must be the named tenant's: its P0, its loaded
        document count, Q queries and the matching size. ValueError otherwise."""
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

    def search_many(self, requests: dict) -> dict:
        """requests: {name: (payloads, min_similarity)} -> {name: [replies]},
        version-2 replies for the tenant's QueryClient.decrypt_replies, its
        queries in order. One library call carries at most max(largest B,
        8192) results (hub_chunks); a tenant alone in a chunk goes through its
        own QueryServer.search_many."""
        plan = {}
        for name, (payloads, min_similarity) in requests.items():
            rec = self._tenant(name)
            s = rec["server"]
            if rec["docs8"] is None:
                raise ValueError(f"tenant {name!r} has no documents loaded")
            pls = [unpack_query(p) for p in payloads]
            try:
                check_query_batch(pls)
            except ValueError as e:
                raise ValueError(f"tenant {name!r}: {e}") from None
            pl = pls[0]
            if pl["P0"] != s.P0 or pl["big"] != s.scheme.k * s.scheme.N:
                raise ValueError(f"tenant {name!r}: query 0 was encrypted under different parameters")
            if pl["D"] != len(s.cq.model.q_w):
                raise ValueError(f"tenant {name!r}: query 0 holds {pl['D']} features, the model {len(s.cq.model.q_w)}")
            ms = thresholds_for(min_similarity, len(pls))
            w, cst, _ = s.plan(None)
            plan[name] = {"payloads": list(payloads), "pls": pls, "ms": ms, "Ts": [s.plan(t)[2] for t in ms],
                          "w": s.engine.to_dev(w), "cst": cst}
        out = {name: [] for name in requests}
        names = list(self.tenants)
        for chunk in hub_chunks({name: (len(plan[name]["pls"]), self.tenants[name]["B"]) for name in plan}):
            if len(chunk) == 1:
                name, rng = chunk[0]
                rec, pn = self.tenants[name], plan[name]
                out[name] += rec["server"].search_many([pn["payloads"][q] for q in rng], rec["docs8"], rec["B"],
                                                       [pn["ms"][q] for q in rng])
                continue
            items, Tcs = [None] * len(names), {}
            for name, rng in chunk:
                rec, pn = self.tenants[name], plan[name]
                eng, pls = rec["server"].engine, pn["pls"]
                body = eng.to_dev(np.stack([pls[q]["body"] for q in rng]))
                ids = eng.to_dev(np.array([pls[q]["id0"] for q in rng], dtype=np.uint64))
                Tcs[name] = [pn["Ts"][q] for q in rng]
                items[names.index(name)] = (body, ids, pls[0]["mask_key"], rec["docs8"], rec["B"], pls[0]["D"],
                                            pn["w"], pn["cst"], Tcs[name], rec["server"].bit_levels)
            res = self.group().search_queries(items)
            for name, rng in chunk:
                ga, gb = res[names.index(name)]
                rec = self.tenants[name]
                reply = pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), rec["B"],
                                     rec["server"].P0, Tcs[name])
                self.check_reply(name, reply, len(rng))
                out[name].append(reply)
        return out
