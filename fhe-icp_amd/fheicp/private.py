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

Key rotation without re-encryption: ``PrivateClient.rotate``
makes the next generation's client with one direct bridge key per resident
old generation; ``encrypt_queries_gens`` encrypts each query once per resident
generation, under that generation's own key; the host keeps every
generation's documents resident (``PrivateServer.load`` / ``append`` /
``rekey``) and ``search_resident`` multiplies generation g's documents by
generation g's GGSWs, then moves the old generations' accumulator rows to the
current key with the grouped bridge (fhe_search_ggsws_gens_batch). The bridge's
noise is added to the product's, never multiplied by the query's norm.

The expected values are the bilinear restatement of fheicp.corpus
(oracle/quant_ref.py, ``corpus_*``); reply format and packing plan are
fheicp.query's.

Query payload (uint64 vector):
    [QUERY_MAGIC, 1, D, P0, base_log | level << 32, N | k << 32,
     GGSW words [c][l][component][coef]]
Document block (uint64 vector):
    [DOCS_MAGIC, 1, B, D, P0, N | k << 32, ceil(B / (N // D)) GLWEs of (k+1)N words]

Seeded payloads (``PrivateClient(..., seeded=True)``): the
body polynomials alone, a third of the full forms; the masks are ChaCha20
streams under the PUBLIC mask key in the payload (4 words = 32 bytes), the
noise came from the client's secret key. GLWE g of a block takes stream id
id0 + g, GGSW row r = c level + l, component c', id0 + r k + c'. An id must not
repeat under one mask key.
Seeded query payload (uint64 vector):
    [SEEDED_QUERY_MAGIC, 1, D, P0, base_log | level << 32, N | k << 32, id0, mask key (4 words),
     (k+1) level bodies of N words [c][l][coef]]
Seeded document block (uint64 vector):
    [SEEDED_DOCS_MAGIC, 1, B, D, P0, N | k << 32, id0, mask key (4 words),
     ceil(B / (N // D)) bodies of N words]
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


def unpack_ggsw_query(arr, copy: bool = True) -> dict:
    """copy=False: "ggsw" is a view of the payload (a reader that uploads it at once)."""
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
            "ggsw": a[HEADER_WORDS:].copy() if copy else a[HEADER_WORDS:]}


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


# ------------------------------------------------ seeded payloads (§8.15) --
SEEDED_QUERY_MAGIC = int.from_bytes(b"FHEICPSQ", "little")
SEEDED_DOCS_MAGIC = int.from_bytes(b"FHEICPSD", "little")
SEEDED_HEADER_WORDS = HEADER_WORDS + 1 + 4       # the v1 header, id0, the mask key


def _mask_key_words(mask_key) -> np.ndarray:
    """A 32-byte mask key (bytes or 8 uint32 words) as the payload's 4 uint64 words."""
    if isinstance(mask_key, (bytes, bytearray)):
        mask_key = np.frombuffer(bytes(mask_key), dtype="<u4")
    k = np.ascontiguousarray(mask_key, dtype=np.uint32).reshape(-1)
    if k.size != 8:
        raise ValueError("a mask key is 32 bytes")
    return k.view(np.uint64).copy()


def pack_ggsw_query_seeded(body, id0: int, mask_key, D: int, P0: int, base_log: int, level: int, N: int,
                           k: int) -> np.ndarray:
    b = np.asarray(body, dtype=np.uint64).reshape(-1)
    head = np.array([SEEDED_QUERY_MAGIC, 1, D, P0, int(base_log) | (int(level) << 32), int(N) | (int(k) << 32),
                     int(id0) % (1 << 64)], np.uint64)
    return np.concatenate([head, _mask_key_words(mask_key), b])


def _seeded_head(arr, magic: int, what: str) -> np.ndarray:
    a = np.asarray(arr)
    if a.dtype != np.uint64 or a.ndim != 1 or a.size < SEEDED_HEADER_WORDS or int(a[0]) != magic:
        raise ValueError(f"not an fheicp seeded {what}")
    if int(a[1]) != 1:
        raise ValueError(f"unsupported seeded {what} version {int(a[1])}")
    return a


def unpack_ggsw_query_seeded(arr, copy: bool = True) -> dict:
    a = _seeded_head(arr, SEEDED_QUERY_MAGIC, "GGSW query payload")
    base_log, level = int(a[4]) & 0xFFFFFFFF, int(a[4]) >> 32
    N, k = int(a[5]) & 0xFFFFFFFF, int(a[5]) >> 32
    D = int(a[2])
    if not 0 < D <= N:
        raise ValueError(f"seeded GGSW query of D = {D} features does not fit one GLWE (N = {N})")
    if a.size != SEEDED_HEADER_WORDS + (k + 1) * level * N:
        raise ValueError("seeded GGSW query payload size does not match its gadget and parameters")
    return {"seeded": True, "D": D, "P0": int(a[3]), "base_log": base_log, "level": level, "N": N, "k": k,
            "id0": int(a[6]), "mask_key": a[7:11].copy().view(np.uint32),
            "body": a[SEEDED_HEADER_WORDS:].copy() if copy else a[SEEDED_HEADER_WORDS:]}


def pack_doc_block_seeded(body, id0: int, mask_key, B: int, D: int, P0: int, N: int, k: int) -> np.ndarray:
    b = np.asarray(body, dtype=np.uint64).reshape(-1)
    head = np.array([SEEDED_DOCS_MAGIC, 1, B, D, P0, int(N) | (int(k) << 32), int(id0) % (1 << 64)], np.uint64)
    return np.concatenate([head, _mask_key_words(mask_key), b])


def unpack_doc_block_seeded(arr) -> dict:
    a = _seeded_head(arr, SEEDED_DOCS_MAGIC, "GLWE document block")
    B, D = int(a[2]), int(a[3])
    N, k = int(a[5]) & 0xFFFFFFFF, int(a[5]) >> 32
    if not 0 < D <= N:
        raise ValueError(f"seeded document block of D = {D} features does not fit one GLWE (N = {N})")
    if a.size != SEEDED_HEADER_WORDS + -(-B // (N // D)) * N:
        raise ValueError("seeded document block size does not match its document count")
    return {"seeded": True, "B": B, "D": D, "P0": int(a[4]), "N": N, "k": k, "id0": int(a[6]),
            "mask_key": a[7:11].copy().view(np.uint32), "body": a[SEEDED_HEADER_WORDS:].copy()}


def _is_seeded(arr, magic: int) -> bool:
    a = np.asarray(arr)
    return a.dtype == np.uint64 and a.ndim == 1 and a.size > 0 and int(a[0]) == magic


def unpack_any_query(arr, copy: bool = True) -> dict:
    """A query payload of either form, dispatched on the magic; "seeded" says which."""
    if _is_seeded(arr, SEEDED_QUERY_MAGIC):
        return unpack_ggsw_query_seeded(arr, copy)
    return dict(unpack_ggsw_query(arr, copy), seeded=False)


def unpack_any_docs(arr) -> dict:
    """A document block of either form, dispatched on the magic; "seeded" says which."""
    if _is_seeded(arr, SEEDED_DOCS_MAGIC):
        return unpack_doc_block_seeded(arr)
    return dict(unpack_doc_block(arr), seeded=False)


def id_ranges_overlap(a0: int, an: int, b0: int, bn: int) -> bool:
    """Whether [a0, a0 + an) and [b0, b0 + bn) meet modulo 2^64 (lengths below 2^64)."""
    M = 1 << 64
    return an > 0 and bn > 0 and ((int(b0) - int(a0)) % M < an or (int(a0) - int(b0)) % M < bn)


def check_query_batch(pls) -> bool:
    """check_ggsw_batch for unpacked payloads of either form; returns whether
    the batch is seeded. One form per batch; seeded queries share one mask key
    and their id ranges [id0, id0 + ggsw_id_span) are disjoint modulo 2^64
    (an id must not repeat under one mask key). ValueError names the query."""
    check_ggsw_batch(pls)
    first = pls[0]
    for i, pl in enumerate(pls[1:], 1):
        if pl["seeded"] != first["seeded"]:
            raise ValueError(f"query {i}: {'a seeded' if pl['seeded'] else 'a full-form'} payload in a batch of "
                             f"{'seeded' if first['seeded'] else 'full-form'} ones")
    if not first["seeded"]:
        return False
    span = ggsw_id_span(first["k"], first["level"])
    for i, pl in enumerate(pls):
        if i and not np.array_equal(pl["mask_key"], first["mask_key"]):
            raise ValueError(f"query {i}: mask key differs from query 0's")
        for j in range(i):
            if id_ranges_overlap(pls[j]["id0"], span, pl["id0"], span):
                raise ValueError(f"query {i}: stream ids [{pl['id0']}, +{span}) overlap query {j}'s under one mask key")
    return True


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

    def __init__(self, corpus: EncryptedCorpus, count: int = 1024, pack_seed=None, enc_seed: int | None = None,
                 seeded: bool = False, mask_seed: int | None = None, in_var: float | None = None):
        """enc_seed: the 64-bit test form of the session's encryption key.
        in_var: the variance (torus units) the packing key is planned for, in
        place of the leveled step's worst case: rotate() passes the product's
        plus the bridge's (params.private_rotation_plan).
        seeded: encrypt_docs / encrypt_query / encrypt_queries emit the seeded
        payloads of DESIGN.md §8.15: masks from the client's own fresh PUBLIC
        mask key (mask_seed: its 64-bit test form), which travels in every
        payload, noise from the secret encryption key, which does not."""
        from .params import extprod_var
        corpus._need()
        scheme = corpus.scheme.with_msg_bits(corpus.P0)
        self.base_log, self.level = self.gadget = plan_gadget(scheme, corpus.cq)
        # the packing plan sees the leveled step's worst-case variance
        if in_var is None:
            in_var = extprod_var(scheme, worst_norm2(corpus.cq), *self.gadget) / 2.0 ** 128
        super().__init__(corpus, count, in_var, pack_seed)
        self.count = int(count)
        # key rotation (§8.19): the clients of the generations this one bridges from,
        # oldest first, their fingerprints and the bridge gadget, once rotate() made this client
        self._sources = []
        self.bridge_gadget = None
        self.bridge_from = None
        self._key_id = None
        self.pack_base_log, self.pack_level = corpus.engine.pack_gadget
        self.base_log, self.level = self.gadget
        self._enc_key = (np.frombuffer(os.urandom(32), np.uint32).copy() if enc_seed is None
                         else corpus.engine.key_from_seed(enc_seed))
        self.seeded = bool(seeded)
        self._mask_key = (np.frombuffer(os.urandom(32), np.uint32).copy() if mask_seed is None
                          else corpus.engine.key_from_seed(mask_seed))
        if self.seeded and np.array_equal(self._mask_key, self._enc_key):
            raise ValueError("the public mask key must differ from the secret encryption key")

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
        if self.seeded:
            i = self._ids(id0)
            body = eng.encrypt_docs_glwe_seeded(dq, self._mask_key, self._enc_key, i)
            return pack_doc_block_seeded(body.cpu().numpy().view(np.uint64), i, self._mask_key, B, D, self.P0,
                                         eng.params.N, eng.params.k)
        glwe = eng.encrypt_docs_glwe(dq, self._enc_key, self._ids(id0))
        return pack_doc_block(glwe.cpu().numpy().view(np.uint64), B, D, self.P0, eng.params.N, eng.params.k)

    def decrypt_docs(self, block) -> np.ndarray:
        """The quantized documents of a block of either form (the key holder's view; tests)."""
        eng = self.corpus.engine
        bl = unpack_any_docs(block)
        eng.set_msg_bits(self.P0)
        S = bl["N"] // bl["D"]
        G = -(-bl["B"] // S)
        glwe = (eng.expand_docs_glwe_seeded(eng.to_dev(bl["body"]), bl["id0"], bl["mask_key"]) if bl["seeded"]
                else eng.to_dev(bl["glwe"]))
        v = eng.decrypt_packed(glwe, G * bl["N"], 0).cpu().numpy().reshape(G, bl["N"])
        return v[:, :S * bl["D"]].reshape(G * S, bl["D"])[:bl["B"]]

    def _encrypt_w(self, W, i: int) -> np.ndarray:
        """The payload of one weight vector under stream id i, in the client's form."""
        eng = self.corpus.engine
        if self.seeded:
            b = eng.encrypt_ggsw_seeded(W, self.base_log, self.level, self._mask_key, self._enc_key, i)
            return pack_ggsw_query_seeded(b.cpu().numpy().view(np.uint64), i, self._mask_key, len(W), self.P0,
                                          self.base_log, self.level, eng.params.N, eng.params.k)
        g = eng.encrypt_ggsw(W, self.base_log, self.level, self._enc_key, i)
        return pack_ggsw_query(g.cpu().numpy().view(np.uint64), len(W), self.P0, self.base_log, self.level,
                               eng.params.N, eng.params.k)

    def encrypt_query(self, q, id0: int | None = None) -> np.ndarray:
        """A reduced query vector -> the GGSW payload sent to the server."""
        eng = self.corpus.engine
        W = self.cq.weights(self.cq.quant(np.asarray(q).reshape(-1)))
        eng.set_msg_bits(self.P0)
        return self._encrypt_w(W, self._ids(id0))

    def encrypt_queries(self, vectors, id0: int | None = None) -> list:
        """Q reduced query vectors [Q, D] -> Q GGSW payloads. One random id0;
        query q takes its (k+1) L k mask ids and (k+1) L noise ids from
        id0 + q (k+1) L k on (ggsw_query_ids), so no id repeats under the
        session key."""
        eng = self.corpus.engine
        qq = self.cq.quant(np.atleast_2d(np.asarray(vectors)))
        ids = ggsw_query_ids(self._ids(id0), len(qq), eng.params.k, self.level)
        eng.set_msg_bits(self.P0)
        return [self._encrypt_w(self.cq.weights(q), i) for q, i in zip(qq, ids)]

    # ------------------------------------------------ key rotation (§8.19) --
    @property
    def key_id(self) -> str:
        """This generation's fingerprint (stored.key_fingerprint of its KSK)."""
        if self._key_id is None:
            from .stored import key_fingerprint
            self._key_id = key_fingerprint(self.corpus.engine.export_key("ksk"))
        return self._key_id

    @property
    def generations(self) -> list:
        """(key_id, client) of every generation this client encrypts queries
        for, oldest first: the clients rotate() bridged from, then itself."""
        return [(c.key_id, c) for c in self._sources] + [(self.key_id, self)]

    def rotate(self, key_seed=None, count: int | None = None, bridge_from=None, device: int | None = None,
               pack_seed=None, bridge_seed=None, noise_seed=None, enc_seed=None, mask_seed=None) -> "PrivateClient":
        """Key rotation without re-encryption -> the next
        generation's client: a new EncryptedCorpus with the same CorpusQuant
        and scheme and fresh keys, one DIRECT bridge key per client of
        bridge_from (oldest first; default [self]; each must still hold its
        secret) in bridge slots 0.., one gadget for all, and a packing key
        planned with the product's and the bridge's variance
        (params.private_rotation_plan). The new client keeps the source
        clients: a query is encrypted once per resident generation, under
        that generation's own key (encrypt_queries_gens). Its eval_keys()
        carry bridge_from (the sources' fingerprints), bridge_gadget and
        bridge_keys (seeded: bridge_key_bodies and bridge_mask_keys). The
        *_seed arguments are the 64-bit test forms; seeded keys and seeded
        payloads carry over."""
        from ._lib import BRIDGE_SLOTS
        from .params import private_rotation_plan
        srcs = [self] if bridge_from is None else list(bridge_from)
        if not 1 <= len(srcs) <= BRIDGE_SLOTS:
            raise ValueError(f"bridge_from names {len(srcs)} generations, a context holds 1 to {BRIDGE_SLOTS} "
                             "bridge keys")
        if len({c.key_id for c in srcs}) != len(srcs):
            raise ValueError("bridge_from names a generation twice")
        for c in srcs:
            c.corpus._need()
        scheme = self.corpus.scheme.with_msg_bits(self.P0)
        gadget, (b, L), in_var = private_rotation_plan(scheme, worst_norm2(self.cq))
        if gadget != self.gadget:
            raise ValueError(f"with a bridge behind it the GGSW gadget becomes {gadget}; the resident documents were "
                             f"packed for {self.gadget}: re-encrypt them (DESIGN.md §8.19)")
        new_corpus = EncryptedCorpus(self.cq, self.corpus.scheme)
        kms = self.corpus.key_mask_seed
        new_corpus.compile(key_seed=key_seed, device=self.corpus.engine.device.index if device is None else device,
                           noise_seed=noise_seed, seeded_keys=self.corpus.seeded_keys,
                           key_mask_seed=None if kms is None else (int(kms) + 16) % 2 ** 64)
        new = PrivateClient(new_corpus, count=self.count if count is None else count, pack_seed=pack_seed,
                            enc_seed=enc_seed, seeded=self.seeded, mask_seed=mask_seed, in_var=in_var)
        for i, c in enumerate(srcs):
            s_old = c.corpus.engine.export_key("s_big")
            new_corpus.engine.keygen_bridge_key(
                s_old, b, L, seed=None if bridge_seed is None else (int(bridge_seed) + i) % 2 ** 64,
                mask_key=new_corpus.next_key_mask() if new_corpus.seeded_keys else None, slot=i)
            s_old[:] = 0
        new._sources = srcs
        new.bridge_gadget = (b, L)
        new.bridge_from = [c.key_id for c in srcs]
        return new

    def eval_keys(self, seeded: bool | None = None) -> dict:
        """QueryClient.eval_keys; after rotate() also key_id, bridge_from (the
        fingerprints of the generations the bridge keys come from, row g of
        bridge_keys from bridge_from[g]), bridge_gadget and bridge_keys
        (seeded: bridge_key_bodies and bridge_mask_keys), for one source too."""
        d = super().eval_keys(seeded)
        if self.bridge_from is None:
            return d
        d["key_id"] = np.array([self.key_id])
        d["bridge_from"] = np.array(self.bridge_from)
        if "bridge_key" in d:
            d["bridge_keys"] = d.pop("bridge_key")[None]
        if "bridge_key_body" in d:
            d["bridge_key_bodies"] = d.pop("bridge_key_body")[None]
            d["bridge_mask_keys"] = d.pop("bridge_mask_key")[None]
        return d

    def encrypt_queries_gens(self, vectors, key_ids=None, id0: int | None = None) -> dict:
        """Q reduced query vectors -> {key_id: Q payloads}: the same quantized
        weights encrypted by each listed generation's own client, under its
        own encryption key (and its own mask key when seeded). key_ids: the
        fingerprints of the generations resident at the host (default: every
        generation of self.generations). Payload formats are encrypt_queries'."""
        gens = dict(self.generations)
        out = {}
        for kid in (list(gens) if key_ids is None else [str(k) for k in key_ids]):
            if kid not in gens:
                raise ValueError(f"no client of generation {kid} is kept (this client holds {', '.join(gens)})")
            out[kid] = gens[kid].encrypt_queries(vectors, id0)
        return out


class PrivateServer(QueryServer):
    """The untrusted host: evaluation keys, the CorpusQuant and P0 only."""

    def __init__(self, eval_keys: dict, cq, P0: int, device: int = 0, scheme=None):
        super().__init__(eval_keys, cq, P0, device, scheme)
        self.base_log, self.level = plan_gadget(self.scheme, cq)
        self._seeded_docs = {}      # mask key bytes -> [(id0, GLWEs, end words)] of the seeded blocks packed so far
        self._init_store(eval_keys)

    # ----------------------- the resident store and key rotation (§8.19) --
    def _init_store(self, eval_keys: dict) -> None:
        # the resident generations, oldest first: {"key_id", "docs" (the operand of search_many), "B"};
        # the current generation, when it holds documents, is last
        self._gens = []
        self._slots = {}            # old generation's fingerprint -> the bridge slot of its key
        self._note_key_id(eval_keys)

    def _note_key_id(self, eval_keys: dict) -> None:
        """Keeps what the current generation's fingerprint comes from and
        nothing else of the dict: its key_id entry, else its ksk words (a few
        MB), else nothing (a seeded dict: the context exports the ksk it
        expanded). The fingerprint itself is worked out on first use."""
        from .stored import _fp
        self._key_id = _fp(eval_keys["key_id"]) if "key_id" in eval_keys else None
        self._ksk = eval_keys.get("ksk") if self._key_id is None else None

    @property
    def key_id(self) -> str:
        """The current generation's fingerprint: the dict's key_id, else that
        of the full-form ksk (a seeded dict's: the key this context expanded)."""
        if self._key_id is None:
            from .stored import key_fingerprint
            self._key_id = key_fingerprint(self._ksk if self._ksk is not None else self.engine.export_key("ksk"))
            self._ksk = None
        return self._key_id

    @property
    def generations(self) -> list:
        """The resident generations, oldest first, as (fingerprint, end)
        pairs: documents end_{g-1} <= b < end_g are under generation g's key."""
        out, end = [], 0
        for g in self._gens:
            end += g["B"]
            out.append((g["key_id"], end))
        return out

    @property
    def old_generations(self) -> list:
        """generations without the current key's."""
        return [(fp, end) for fp, end in self.generations if fp != self.key_id]

    def load(self, block) -> int:
        """Make a document block (under the CURRENT key) the resident store,
        in place of whatever was resident; -> the resident count."""
        docs, B = self.pack_docs_many(block)
        if B < 1:
            raise ValueError("an empty document store")
        for s in self.engine.bridge_slots():  # the old generations' keys serve nothing any more
            self.engine.drop_bridge_key(s)
        self._gens, self._slots = [{"key_id": self.key_id, "docs": docs, "B": int(B)}], {}
        return int(B)

    def append(self, block) -> int:
        """Add a block encrypted under the CURRENT key after the resident
        documents; -> the resident count. The block becomes whole GLWEs of the
        current generation's operand, so it continues a generation only at a
        GLWE boundary: after B documents with B % (N // D) == 0 (ValueError
        otherwise; a rotation starts a new operand)."""
        import torch
        if not self._gens:
            return self.load(block)
        cur = self._gens[-1] if self._gens[-1]["key_id"] == self.key_id else None
        S = self.scheme.N // len(self.cq.model.q_w)
        if cur is not None and cur["B"] % S:
            raise ValueError(f"the current generation holds {cur['B']} documents, its last GLWE is partly filled "
                             f"({S} documents per GLWE): a block continues a generation only at a GLWE boundary")
        docs, B = self.pack_docs_many(block)
        if B < 1:
            raise ValueError("an empty document block")
        if cur is None:
            self._gens.append({"key_id": self.key_id, "docs": docs, "B": int(B)})
        else:
            cur["docs"], cur["B"] = torch.cat([cur["docs"], docs]).contiguous(), cur["B"] + int(B)
        return self.generations[-1][1]

    def rekey(self, eval_keys: dict) -> None:
        """Key rotation: install the next generation's evaluation keys and
        bridge keys (PrivateClient.rotate(...).eval_keys()). Every resident
        document becomes old-generation. The dict must hold a bridge key from
        EVERY resident generation, the one that was current until now
        included: ValueError naming the missing fingerprint, before anything
        changes. Row g of bridge_keys goes into slot g; slots whose generation
        is not resident are dropped. The single-bridge dict (bridge_key,
        bridge_from one fingerprint) is accepted too."""
        if "pack_key" not in eval_keys and "pack_key_body" not in eval_keys:
            raise ValueError("the evaluation keys hold no packing key")
        many = "bridge_keys" in eval_keys or "bridge_key_bodies" in eval_keys
        single = "bridge_key" in eval_keys or "bridge_key_body" in eval_keys
        if (many or single) and "bridge_from" not in eval_keys:
            raise ValueError("the evaluation keys hold bridge keys and no bridge_from")
        src = [str(f) for f in np.asarray(eval_keys["bridge_from"]).reshape(-1)] if many or single else []
        for g in self._gens:
            if g["key_id"] not in src:
                raise ValueError(f"documents under key {g['key_id']} are resident and the evaluation keys hold no "
                                 f"bridge key from it (they bridge from {', '.join(src) or 'no generation'})")
        eng = self.engine
        eng.import_eval_keys(eval_keys)  # row g into slot g (the single form: slot 0)
        self.bit_levels = int(np.asarray(eval_keys.get("pack_bit_levels", [0])).reshape(-1)[0])
        self._slots = {g["key_id"]: src.index(g["key_id"]) for g in self._gens}
        for s in [s for s in eng.bridge_slots() if s not in self._slots.values()]:
            eng.drop_bridge_key(s)
        self._note_key_id(eval_keys)

    def _upload_words(self, parts):
        """uint64 host vectors -> one device tensor, each part copied straight
        into its place (no concatenated host copy)."""
        import torch
        parts = [np.ascontiguousarray(a, dtype=np.uint64) for a in parts]
        out = torch.empty(sum(a.size for a in parts), dtype=torch.int64, device=self.engine.device)
        at = 0
        for a in parts:
            out[at:at + a.size].copy_(torch.from_numpy(a.view(np.int64)))
            at += a.size
        return out

    def search_resident(self, bundle: dict, min_similarity=None) -> list:
        """bundle: {key_id: Q payloads}, what PrivateClient.encrypt_queries_gens
        returns: every query once per resident generation, under that
        generation's key. Generation g's documents meet generation g's GGSWs
        and the old generations' rows are bridged to the current key, one
        fhe_search_ggsws_gens_batch per chunk of query_chunks(Q, B) -> a LIST
        of version-2 replies over all resident documents, oldest generation
        first, for the CURRENT client's decrypt_replies. A bundle that lacks a
        resident generation is refused by its fingerprint; each generation's
        payloads pass check_query_batch on their own (one form per generation)."""
        from .query import pack_replies, query_chunks, thresholds_for
        if not self._gens:
            raise RuntimeError("no resident documents: call load() first")
        eng = self.engine
        gens = []
        for g in self._gens:
            fp = g["key_id"]
            if fp not in bundle:
                raise ValueError(f"documents under key {fp} are resident and the bundle holds no queries for it "
                                 f"(it holds {', '.join(str(k) for k in bundle) or 'none'})")
            try:
                # views, not copies: a bundle carries G times a batch's GGSW words and each is uploaded once
                pls = [unpack_any_query(p, copy=False) for p in bundle[fp]]
                seeded = check_query_batch(pls)
                self._check(pls[0], "query 0")
                if (pls[0]["base_log"], pls[0]["level"]) != (self.base_log, self.level):
                    raise ValueError("query 0: gadget differs from the one the documents were packed for")
            except ValueError as e:
                raise ValueError(f"generation {fp}: {e}") from None
            if gens and len(pls) != len(gens[0][1]):
                raise ValueError(f"generation {fp}: {len(pls)} queries, generation {gens[0][0]['key_id']} "
                                 f"{len(gens[0][1])}")
            gens.append((g, pls, seeded))
        Q, D = len(gens[0][1]), gens[0][1][0]["D"]
        B = self.generations[-1][1]
        _, cst, _ = self.plan(None)
        Ts = [self.plan(t)[2] for t in thresholds_for(min_similarity, Q)]
        out = []
        for ch in query_chunks(Q, B):
            Tc = [Ts[q] for q in ch]
            items = []
            for g, pls, seeded in gens:
                if seeded:   # expanded on this context; the generations entry takes full forms
                    b = self._upload_words(pls[q]["body"] for q in ch)
                    w = eng.expand_ggsws_seeded(b, [pls[q]["id0"] for q in ch], self.base_log, self.level,
                                                pls[0]["mask_key"])
                else:
                    w = self._upload_words(pls[q]["ggsw"] for q in ch)
                slot = -1 if g["key_id"] == self.key_id else self._slots[g["key_id"]]
                items.append((slot, w, g["docs"], g["B"]))
            ga, gb = eng.search_ggsws_gens(items, self.base_log, self.level, D, cst, Tc, self.bit_levels)
            out.append(pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, self.P0,
                                    Tc))
        return out

    def _note_seeded_docs(self, bl: dict) -> None:
        """An id must not repeat under one mask key: a seeded block whose ids
        [id0, id0 + G) meet those of ANOTHER block packed under the same mask
        key is refused (the same block packed again, for the other operand,
        is the same ciphertexts and passes). A courtesy of the host, not the
        defence: the client owns its ids."""
        G = -(-bl["B"] // (bl["N"] // bl["D"]))
        # the block's first and last body words tell it from another block (bodies are pseudorandom)
        rec = (bl["id0"], G, bl["body"][:4].tobytes() + bl["body"][-4:].tobytes())
        seen = self._seeded_docs.setdefault(bl["mask_key"].tobytes(), [])
        if rec in seen:
            return
        for id0, n, _ in seen:
            if id_ranges_overlap(id0, n, rec[0], G):
                raise ValueError(f"document block: stream ids [{rec[0]}, +{G}) overlap those of a block already "
                                 f"packed under the same mask key ([{id0}, +{n}))")
        seen.append(rec)

    def _docs_operand(self, block, queries: bool):
        bl = unpack_any_docs(block)
        self._check(bl, "document block")
        eng = self.engine
        if bl["seeded"]:
            self._note_seeded_docs(bl)
            return eng.pack_docs_glwe_seeded(eng.to_dev(bl["body"]), bl["id0"], bl["mask_key"], bl["B"], bl["D"],
                                             self.base_log, self.level, queries=queries), bl["B"]
        pack = eng.pack_docs_glwe_queries if queries else eng.pack_docs_glwe
        return pack(eng.to_dev(bl["glwe"]), bl["B"], bl["D"], self.base_log, self.level), bl["B"]

    def _check(self, pl: dict, what: str) -> None:
        if pl["P0"] != self.P0 or pl["N"] != self.scheme.N or pl["k"] != self.scheme.k:
            raise ValueError(f"{what} was encrypted under different parameters")
        if pl["D"] != len(self.cq.model.q_w):
            raise ValueError(f"{what} holds {pl['D']} features, the model {len(self.cq.model.q_w)}")

    def pack_docs(self, block):
        """A document block of either form -> (the device-resident digit
        operand, B). A seeded block is never expanded: the operand is made
        from its bodies (fhe_glwe_docs_pack_seeded)."""
        return self._docs_operand(block, False)

    def search(self, payload, docs8, B: int, min_similarity: float | None) -> np.ndarray:
        """One GGSW query against B packed encrypted documents -> the reply."""
        eng = self.engine
        pl = unpack_any_query(payload)
        self._check(pl, "query")
        if (pl["base_log"], pl["level"]) != (self.base_log, self.level):
            raise ValueError("query gadget differs from the one the documents were packed for")
        _, cst, T = self.plan(min_similarity)
        if pl["seeded"]:
            ga, gb = eng.search_ggsw_seeded(eng.to_dev(pl["body"]), pl["id0"], pl["mask_key"], self.base_log,
                                            self.level, docs8, int(B), pl["D"], cst, T, self.bit_levels)
        else:
            ga, gb = eng.search_ggsw(eng.to_dev(pl["ggsw"]), self.base_log, self.level, docs8, int(B), pl["D"], cst,
                                     T, self.bit_levels)
        return pack_reply(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, self.P0, T)

    # -------------------------------------------------- batches of queries --
    def pack_docs_many(self, block):
        """A document block of either form -> (the device-resident operand of
        search_many, B); seeded blocks as in pack_docs
        (fhe_glwe_docs_queries_pack_seeded)."""
        return self._docs_operand(block, True)

    def search_many(self, payloads, docs, B: int, min_similarity=None) -> list:
        """Q GGSW queries of one key holder, all full form or all seeded
        (check_query_batch), against B encrypted documents
        packed by pack_docs_many, in one pass (fhe_search_ggsws_batch) -> a
        LIST of version-2 replies (query.pack_replies), one per chunk of
        query_chunks(Q, B). min_similarity: a float, None, or a sequence of Q
        of them. QueryClient.decrypt_replies takes the list."""
        from .query import pack_replies, query_chunks, thresholds_for
        eng = self.engine
        pls = [unpack_any_query(p) for p in payloads]
        seeded = check_query_batch(pls)
        self._check(pls[0], "query 0")
        if (pls[0]["base_log"], pls[0]["level"]) != (self.base_log, self.level):
            raise ValueError("query 0: gadget differs from the one the documents were packed for")
        Q, D = len(pls), pls[0]["D"]
        _, cst, _ = self.plan(None)
        Ts = [self.plan(t)[2] for t in thresholds_for(min_similarity, Q)]
        out = []
        for ch in query_chunks(Q, int(B)):
            Tc = [Ts[q] for q in ch]
            if seeded:
                b = eng.to_dev(np.concatenate([pls[q]["body"] for q in ch]))
                ga, gb = eng.search_ggsws_seeded(b, [pls[q]["id0"] for q in ch], pls[0]["mask_key"], self.base_log,
                                                 self.level, docs, int(B), D, cst, Tc, self.bit_levels)
            else:
                g = eng.to_dev(np.concatenate([pls[q]["ggsw"] for q in ch]))
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
    one GPU; each tenant's blocks and queries in either form, full or seeded
    (DESIGN.md §8.15), mixed freely between tenants of one call. The host learns which tenant asked, Q and B; documents, queries
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
                pls = [unpack_any_query(p) for p in payloads]
                check_query_batch(pls)
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
                if pls[0]["seeded"]:    # expanded on the tenant's own context; the group entry takes full forms
                    b = s.engine.to_dev(np.concatenate([pls[q]["body"] for q in rng]))
                    g = s.engine.expand_ggsws_seeded(b, [pls[q]["id0"] for q in rng], s.base_log, s.level,
                                                     pls[0]["mask_key"])
                else:
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
