"""Stored-ciphertext search with two parties.

The stored-ciphertext mode (fheicp.corpus: documents kept as seeded LWEs and
searched without decryption) with its two roles in two contexts:

  * CorpusClient, the key holder: encrypts documents (EncryptedCorpus's
    encrypt_docs / payloads), hands out evaluation keys with a packing key and
    decrypts replies; rotate() makes the next generation's client with a
    bridge key, so the host keeps searching the documents stored under the
    old key without re-encryption;
  * CorpusServer, the host: holds evaluation keys, the public mask key, the
    CorpusQuant and P0 only. It keeps a client's encrypted documents resident
    and scores Q CLEAR queries against them in one pass per chunk
    (fhe_search_seeded_queries_batch), answering with packed GLWEs that only
    the client can open.

The host sees the queries, the thresholds, Q, B and D; it never sees a
document, a score or a threshold bit. Replies are the version-2 format of
fheicp.query (pack_replies / unpack_replies) unchanged; the width field
carries the chunk's own width P <= P0 (EncryptedCorpus.plan_many).

CorpusHub puts several key holders, each with its own
CorpusServer, behind one GPU: a call that names several of them runs their
sign extractions in one group launch sequence, key rotation included.
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


def key_fingerprint(ksk) -> str:
    """16 hex digits naming a key generation: sha256 over the KSK words (public
    evaluation-key material, different for every secret key)."""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(ksk, dtype=np.uint64).tobytes()).hexdigest()[:16]


def _fp(v) -> str:
    """A fingerprint entry of an evaluation-key dict (str or a numpy string array) -> str."""
    return str(np.asarray(v).reshape(-1)[0])


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

    def __init__(self, corpus: EncryptedCorpus, count: int = 1024, in_var: float | None = None, pack_seed=None,
                 extra_var: float = 0.0, next_id: int | None = None):
        """Generates the packing key planned once at P0 (at P < P0 the margin
        2^(63 - P) / sigma only grows) for replies of up to `count` results per
        GLWE. in_var defaults to leveled_in_var, the l1 bound of this mode's
        weights (pack_seed: the 64-bit test form). extra_var (torus units) is
        added to the plan's input variance: rotate() passes the bridge's.
        next_id: where this client's default stream ids start (rotate()
        continues after the old client's; None: random ids)."""
        from .params import pack_plan, pack_sigmas
        corpus._need()
        self.corpus = corpus
        self.cq, self.P0 = corpus.cq, corpus.P0
        scheme = corpus.scheme.with_msg_bits(self.P0)
        self.count = int(count)
        self.in_var = leveled_in_var(self.cq, self.P0, scheme) if in_var is None else float(in_var)
        self.pack_in_var = self.in_var + float(extra_var)
        self.base_log, self.level, self.bit_levels = pack_plan(scheme, count, self.pack_in_var)
        #: the plan's margin in sigmas (below 9.2 when no gadget reaches the bar)
        self.margin = pack_sigmas(scheme, count, self.pack_in_var, self.base_log, self.level, 63 - self.P0)
        corpus.engine.keygen_pack(self.base_log, self.level, seed=pack_seed,
                                  mask_key=corpus.next_key_mask() if corpus.seeded_keys else None)
        self.next_id = None if next_id is None else int(next_id) % 2 ** 64
        self._id_end = 0 if next_id is None else self.next_id  # one past the largest stream id handed out
        self.bridge_gadget = None  # (base_log, level) of the bridge key and the fingerprint of the
        self.bridge_from = None    # generation it comes from, once rotate() made this client
        self._key_id = None

    def _note_ids(self, ids, D: int) -> None:
        if len(ids):
            self._id_end = max(self._id_end, int(np.max(ids)) + int(D))

    def encrypt_docs(self, docs, id0=None):
        """EncryptedCorpus.encrypt_docs; a rotated client's default ids are
        consecutive runs of D after every id of the generations before it."""
        docs = np.ascontiguousarray(docs)
        B, D = docs.shape
        if id0 is None and self.next_id is not None:
            id0 = (np.uint64(self.next_id) + np.arange(B, dtype=np.uint64) * np.uint64(D))
            self.next_id = (self.next_id + B * D) % 2 ** 64
        bodies, ids = self.corpus.encrypt_docs(docs, id0)
        self._note_ids(ids, D)
        return bodies, ids

    @property
    def id_end(self) -> int:
        """One past the largest stream id this client (or, for a rotated
        client, any generation before it) has handed out, modulo 2^64."""
        return self._id_end % 2 ** 64

    @property
    def key_id(self) -> str:
        """This generation's fingerprint (key_fingerprint of its KSK)."""
        if self._key_id is None:
            self._key_id = key_fingerprint(self.corpus.engine.export_key("ksk"))
        return self._key_id

    def rotate(self, key_seed=None, count: int | None = None, bridge_from=None,
               device: int | None = None, pack_seed=None, bridge_seed=None, noise_seed=None) -> "CorpusClient":
        """Key rotation without re-encryption -> the next
        generation's client: a new EncryptedCorpus with the same CorpusQuant,
        scheme and mask key and fresh keys, a bridge key from bridge_from's
        big key (default: this client; it must still hold its secret) to the
        new one, and a packing key planned with the bridge's variance added.
        Its eval_keys() carry bridge_key, bridge_gadget and bridge_from; its
        default stream ids continue after this client's. The *_seed arguments
        are the 64-bit test forms. When this client's keys are seeded (§8.16)
        so are the new generation's and its bridge key, under mask keys of
        their own.

        bridge_from may also be a SEQUENCE of clients, oldest first: every
        generation whose documents are still resident. The
        new client then holds one DIRECT bridge key per client, each under its
        own fresh keys (bridge_seed + i in the test form), one gadget for all,
        and its eval_keys() carry bridge_from as an array of their
        fingerprints and bridge_keys [G, words] (seeded: bridge_key_bodies and
        bridge_mask_keys). A row still passes one bridge, so the packing plan
        is the single bridge's."""
        from .params import bridge_plan, bridge_var
        many = bridge_from is not None and not isinstance(bridge_from, CorpusClient)
        srcs = list(bridge_from) if many else [self if bridge_from is None else bridge_from]
        if many:
            from ._lib import BRIDGE_SLOTS
            if not 1 <= len(srcs) <= BRIDGE_SLOTS:
                raise ValueError(f"bridge_from names {len(srcs)} generations, a context holds 1 to {BRIDGE_SLOTS} "
                                 "bridge keys")
            if len({c.key_id for c in srcs}) != len(srcs):
                raise ValueError("bridge_from names a generation twice")
        for c in srcs:
            c.corpus._need()
        src = srcs[0]
        old = src.corpus.engine
        scheme = self.corpus.scheme.with_msg_bits(self.P0)
        new_corpus = EncryptedCorpus(self.cq, self.corpus.scheme)
        dev = old.device.index if device is None else device
        kms = self.corpus.key_mask_seed
        new_corpus.compile(key_seed=key_seed, device=dev, mask_key=self.corpus.mask_key, noise_seed=noise_seed,
                           seeded_keys=self.corpus.seeded_keys,
                           key_mask_seed=None if kms is None else (int(kms) + 16) % 2 ** 64)
        b, L = bridge_plan(scheme, self.in_var)
        new = CorpusClient(new_corpus, count=self.count if count is None else count, in_var=self.in_var,
                           pack_seed=pack_seed, extra_var=bridge_var(scheme, b, L) / 2.0 ** 128,
                           next_id=max([self.id_end] + [c.id_end for c in srcs]))
        for i, c in enumerate(srcs):
            s_old = c.corpus.engine.export_key("s_big")
            new_corpus.engine.keygen_bridge_key(
                s_old, b, L, seed=None if bridge_seed is None else (int(bridge_seed) + i) % 2 ** 64,
                mask_key=new_corpus.next_key_mask() if new_corpus.seeded_keys else None, slot=i)
            s_old[:] = 0
        new.bridge_gadget = (b, L)
        new.bridge_from = [c.key_id for c in srcs] if many else src.key_id
        return new

    def payloads(self, bodies, ids):
        return self.corpus.payloads(bodies, ids)

    def eval_keys(self, seeded: bool | None = None) -> dict:
        """What the host gets: bsk, ksk, the gadgets' keys, the packing key
        with its gadget and the bit prefix, and this generation's fingerprint
        (key_id); after rotate() also bridge_key, bridge_gadget and
        bridge_from, the old generation's fingerprint. No secret key. On a
        corpus compiled with seeded_keys the dict is the seeded form (§8.16);
        eval_keys(seeded=False) is the full form of the same keys. key_id is
        the fingerprint of the full-form ksk in both."""
        d = self.corpus.engine.export_eval_keys(seeded=self.corpus.seeded_keys if seeded is None else seeded)
        d["pack_bit_levels"] = np.array([self.bit_levels], dtype=np.int64)
        d["key_id"] = np.array([self.key_id])
        if isinstance(self.bridge_from, list):
            # the multi-bridge form (§8.17), for one named generation too
            d["bridge_from"] = np.array(self.bridge_from)
            if "bridge_key" in d:
                d["bridge_keys"] = d.pop("bridge_key")[None]
            if "bridge_key_body" in d:
                d["bridge_key_bodies"] = d.pop("bridge_key_body")[None]
                d["bridge_mask_keys"] = d.pop("bridge_mask_key")[None]
        elif self.bridge_from is not None:
            d["bridge_from"] = np.array([self.bridge_from])
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
        if "pack_key" not in eval_keys and "pack_key_body" not in eval_keys:
            raise ValueError("the evaluation keys hold no packing key")
        self.cq, self.P0 = cq, int(P0)
        self._plan = EncryptedCorpus(cq, scheme)  # planning only: never compiled, holds no key
        if self._plan.P0 != self.P0:
            raise ValueError(f"P0 = {self.P0} does not match the model's worst-case width {self._plan.P0}")
        self.scheme = self._plan.scheme
        self.mask_key = np.ascontiguousarray(mask_key, dtype=np.uint32).reshape(8).copy()
        self.engine = self._make_engine(device)
        self.engine.import_eval_keys(eval_keys)
        self.bit_levels = int(np.asarray(eval_keys.get("pack_bit_levels", [0])).reshape(-1)[0])
        self.body = self.ids = None
        # key rotation (§8.12): the resident documents b < b_old are under the
        # generation old_key_id and go through the bridge key
        self.key_id = self._key_id_of(eval_keys)
        self.b_old = 0
        self.old_key_id = None
        # several old generations resident (§8.17): their (fingerprint, end)
        # pairs, oldest first, and the bridge slot of each; None with fewer
        # than two, where b_old and old_key_id say it all
        self._old_gens = None
        self._gen_slots = None

    @property
    def old_generations(self) -> list:
        """The resident old generations, oldest first, as (fingerprint, end)
        pairs: documents end_{g-1} <= b < end_g are under generation g's key."""
        if self._old_gens:
            return list(self._old_gens)
        return [(self.old_key_id, int(self.b_old))] if self.b_old else []

    @property
    def generations(self) -> list:
        """old_generations and, when documents under the current key are
        resident, (key_id, B) last."""
        gens = self.old_generations
        B = 0 if self.body is None else int(self.body.shape[0])
        if B > (gens[-1][1] if gens else 0):
            gens.append((self.key_id, B))
        return gens

    def _reset_generations(self) -> None:
        if self._old_gens:  # the extra slots' keys serve nothing any more
            for slot in [s for s in self.engine.bridge_slots() if s > 0]:
                self.engine.drop_bridge_key(slot)
        self._old_gens = self._gen_slots = None

    def _key_id_of(self, eval_keys: dict) -> str:
        """The generation's fingerprint: the dict's key_id, else that of the
        full-form ksk (a seeded dict's: the key this context just expanded)."""
        if "key_id" in eval_keys:
            return _fp(eval_keys["key_id"])
        return key_fingerprint(eval_keys["ksk"] if "ksk" in eval_keys else self.engine.export_key("ksk"))

    def _make_engine(self, device):
        from .engine import Engine
        return Engine(self.scheme, device)

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
        self._reset_generations()
        self.b_old, self.old_key_id = 0, None
        return int(ids.size)

    def _check_docs(self, bodies, ids):
        bodies = np.ascontiguousarray(bodies, dtype=np.uint64)
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if bodies.ndim != 2 or bodies.shape[0] != ids.size or bodies.shape[0] < 1:
            raise ValueError("needs bodies [B, D] and B stream ids, B >= 1")
        if bodies.shape[1] != len(self.cq.model.q_w):
            raise ValueError(f"documents hold {bodies.shape[1]} features, the model {len(self.cq.model.q_w)}")
        return bodies, ids

    def append(self, bodies, ids) -> int:
        """Add documents encrypted under the CURRENT key after the resident
        ones (old-generation documents stay first); -> the resident count."""
        import torch
        if self.body is None:
            return self.load(bodies, ids)
        bodies, ids = self._check_docs(bodies, ids)
        self.body = torch.cat([self.body, self.engine.to_dev(bodies)]).contiguous()
        self.ids = torch.cat([self.ids, self.engine.to_dev(ids)]).contiguous()
        return int(self.ids.shape[0])

    def rekey(self, eval_keys: dict) -> None:
        """Key rotation (§8.12): install the next generation's evaluation keys
        and bridge key (CorpusClient.rotate(...).eval_keys()). Every resident
        document becomes old-generation. One old generation is resident at a
        time: with old-generation documents already resident, the bridge must
        come from THEIR generation (rotate(bridge_from=...)) and every
        resident document must be of it.

        A multi-bridge dict (rotate(bridge_from=[clients]), §8.17) lifts that:
        it must hold a bridge for EVERY resident generation, the one that was
        current until now included (ValueError naming the missing fingerprint,
        before anything changes). Each bridge goes into a slot; slots whose
        generation is not resident are dropped."""
        if "pack_key" not in eval_keys and "pack_key_body" not in eval_keys:
            raise ValueError("the evaluation keys hold no packing key")
        B = 0 if self.body is None else int(self.body.shape[0])
        if "bridge_keys" in eval_keys or "bridge_key_bodies" in eval_keys:
            return self._rekey_many(eval_keys, B)
        if B and self._old_gens:
            raise ValueError(f"documents of {len(self._old_gens)} old generations are resident and the evaluation "
                             "keys hold one bridge key: rotate(bridge_from=[...]) makes one per generation")
        if B:
            if ("bridge_key" not in eval_keys and "bridge_key_body" not in eval_keys) or "bridge_from" not in eval_keys:
                raise ValueError("documents are resident and the evaluation keys hold no bridge key")
            src = _fp(eval_keys["bridge_from"])
            if self.b_old > 0:
                if src != self.old_key_id:
                    raise ValueError(f"old-generation documents of key {self.old_key_id} are resident; the bridge "
                                     f"key comes from {src} (rotate(bridge_from=...) needs their generation)")
                if self.b_old != B:
                    raise ValueError("documents of two generations are resident: no chained bridges, reload the "
                                     "newer ones under the new key")
            elif src != self.key_id:
                raise ValueError(f"the resident documents are under key {self.key_id}; the bridge key comes "
                                 f"from {src}")
        self.engine.import_eval_keys(eval_keys)
        self.bit_levels = int(np.asarray(eval_keys.get("pack_bit_levels", [0])).reshape(-1)[0])
        if B and self.b_old == 0:
            self.old_key_id = self.key_id
        self.b_old = B
        self.key_id = self._key_id_of(eval_keys)

    def _rekey_many(self, eval_keys: dict, B: int) -> None:
        """rekey with a multi-bridge dict: bridge_from[g]'s key is row g."""
        if "bridge_from" not in eval_keys:
            raise ValueError("the evaluation keys hold bridge keys and no bridge_from")
        src = [str(f) for f in np.asarray(eval_keys["bridge_from"]).reshape(-1)]
        resident = [(fp, end) for fp, end in self.generations] if B else []
        for fp, _ in resident:
            if fp not in src:
                raise ValueError(f"documents under key {fp} are resident and the evaluation keys hold no bridge "
                                 f"key from it (they bridge from {', '.join(src)})")
        eng = self.engine
        eng.import_eval_keys(eval_keys)  # row g into slot g, the slots after them dropped
        self.bit_levels = int(np.asarray(eval_keys.get("pack_bit_levels", [0])).reshape(-1)[0])
        slots = [src.index(fp) for fp, _ in resident]
        if len(resident) == 1 and slots[0] != 0:
            # one old generation runs the single bridge, which reads slot 0
            g, (b, L) = slots[0], (int(x) for x in np.asarray(eval_keys["bridge_gadget"]).reshape(2))
            if "bridge_keys" in eval_keys:
                eng.import_bridge_key(b, L, np.asarray(eval_keys["bridge_keys"])[g], slot=0)
            else:
                eng.import_bridge_key_seeded(b, L, np.asarray(eval_keys["bridge_mask_keys"])[g],
                                             np.asarray(eval_keys["bridge_key_bodies"])[g], slot=0)
            slots = [0]
        for s in [s for s in range(len(src)) if s not in slots]:
            eng.drop_bridge_key(s)
        if len(resident) >= 2:
            self._old_gens, self._gen_slots = resident, slots
            self.b_old, self.old_key_id = B, None
        else:
            self._old_gens = self._gen_slots = None
            self.b_old, self.old_key_id = B, (resident[0][0] if resident else None)
        self.key_id = self._key_id_of(eval_keys)

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
            if self._old_gens:  # several old generations: one grouped bridge over their rows (§8.17)
                ga, gb = eng.search_seeded_queries_gens(self.body, self.ids, self.mask_key, eng.to_dev(Wr), cst, Ts,
                                                        self.bit_levels, gen_ends=[e for _, e in self._old_gens],
                                                        gen_slots=self._gen_slots)
            else:
                ga, gb = eng.search_seeded_queries(self.body, self.ids, self.mask_key, eng.to_dev(Wr), cst, Ts,
                                                   self.bit_levels, b_old=self.b_old)
            out.append(pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64), B, P, Ts))
        return out

    def search(self, query, min_similarity=None) -> np.ndarray:
        """One query: the single reply of search_many([query])."""
        return self.search_many(np.asarray(query).reshape(1, -1), min_similarity)[0]


# ------------------------------------------------------ several key holders --
# One evaluation-only host serving tenants that each hold their own keys and
# their own STORED documents: every tenant keeps a
# CorpusServer; a call that names several of them runs their sign extractions
# in one group launch sequence (fhe_search_seeded_queries_group_batch) and
# answers each tenant in the version-2 reply format.
def group_form(scheme, P: int) -> bool:
    """Whether a group of contexts of `scheme` at width P exists
    (fhe_group_form, host only): False where a round of the sign schedule
    runs the classic rotation (P = 27)."""
    from . import _lib
    import ctypes as C
    rc = _lib.lib().fhe_group_form(C.byref(_lib.params_struct(scheme.with_msg_bits(int(P)).as_dict())))
    if rc < 0:
        _lib.check(rc)
    return rc == 1


def corpus_rounds(requests: dict, plans: dict, sizes: dict, group_ok=None, cap: int | None = None) -> list:
    """The rounds of one CorpusHub.search_many call, as pure planning (no
    device). requests: {name: (queries, min_similarity)}; plans: {name: the
    tenant's EncryptedCorpus planning object}; sizes: {name: B}.

    Round i takes chunk i of each tenant's query_chunks(Q, B), split further
    by hub_chunks' bound on the results of one library call. Each piece is
    planned at its own width P_t (plan_many); the round's width is P = max P_t
    and a piece's weight rows take the exact arithmetic shift >> (P - P_t)
    (its rows carry 2^(P0 - P_t), the round's 2^(P0 - P)). A piece alone in
    its round, or a round whose width has no group form (group_ok(P) False),
    goes through the tenants' own servers.

    -> [{"mode": "group" | "own", "P": P, "parts": [{"name", "queries" (a
    range into the tenant's queries), "W" int64 [q, D], "cst", "Ts", "P_t"}]}]
    """
    from .query import MAX_RESULTS, hub_chunks
    cap = MAX_RESULTS if cap is None else int(cap)
    qs, ts, chunks = {}, {}, {}
    for name, (queries, min_similarity) in requests.items():
        q = np.atleast_2d(np.asarray(queries))
        qs[name], ts[name] = q, thresholds_for(min_similarity, q.shape[0])
        chunks[name] = query_chunks(q.shape[0], int(sizes[name]), cap)
    rounds = []
    for i in range(max((len(c) for c in chunks.values()), default=0)):
        live = {name: c[i] for name, c in chunks.items() if i < len(c)}
        for piece in hub_chunks({name: (len(r), int(sizes[name])) for name, r in live.items()}, cap):
            parts = []
            for name, sub in piece:
                rng = range(live[name].start + sub.start, live[name].start + sub.stop)
                Wr, cst, Ts, P_t = plans[name].plan_many(qs[name][rng.start:rng.stop], [ts[name][q] for q in rng])
                parts.append({"name": name, "queries": rng, "W": Wr, "cst": cst, "Ts": Ts, "P_t": int(P_t)})
            P = max(p["P_t"] for p in parts)
            ok = len(parts) > 1 and (group_ok(P) if group_ok is not None
                                     else group_form(plans[parts[0]["name"]].scheme, P))
            if ok:
                for p in parts:
                    p["W"] = p["W"] >> np.int64(P - p["P_t"])
            rounds.append({"mode": "group" if ok else "own", "P": P, "parts": parts})
    return rounds


class CorpusHub:
    """Tenants with their own keys and their own stored (encrypted) documents
    behind one GPU. The host learns which tenant asked, the queries and the
    thresholds; each tenant's documents, scores and bits stay under its key."""

    def __init__(self, device: int = 0, rotation_schedules: bool = False):
        """rotation_schedules: tenants may keep several old generations
        resident (§8.18): rekey takes a multi-bridge dict and every group
        round bridges all tenants' old generations in one grouped pass
        (fhe_search_seeded_queries_group_gens_batch). The default keeps one
        old generation per tenant and the per-tenant bridge of §8.13."""
        self.device = device
        self.rotation_schedules = bool(rotation_schedules)
        self.tenants = {}  # name -> CorpusServer
        self._group = None

    def add_tenant(self, name, eval_keys, cq, P0: int, mask_key, scheme=None, server=None):
        """Builds the tenant's CorpusServer from its evaluation keys. Every
        tenant shares the first one's P0 and scheme parameters: ValueError
        naming the tenant otherwise. `server` is for tests only: it adopts a
        ready (or stub) server in place of building one, so the checks run
        without a device."""
        if name in self.tenants:
            raise ValueError(f"tenant {name!r} is already registered")
        if server is None:
            plan = EncryptedCorpus(cq, scheme)  # planning only: the width and the scheme this model needs
            p0, want = int(P0), plan.scheme
            if plan.P0 != p0:
                raise ValueError(f"tenant {name!r}: P0 = {p0} does not match the model's worst-case width {plan.P0}")
        else:
            p0, want = int(server.P0), server.scheme
        for other, s in self.tenants.items():
            if int(s.P0) != p0:
                raise ValueError(f"tenant {name!r}: P0 = {p0} differs from tenant {other!r}'s {int(s.P0)}")
            if s.scheme != want:
                raise ValueError(f"tenant {name!r}: scheme parameters differ from tenant {other!r}'s")
            break
        if server is None:
            server = CorpusServer(eval_keys, cq, p0, mask_key, self.device, scheme)
        self.tenants[name] = server
        self._drop_group()
        return server

    def _drop_group(self) -> None:
        if self._group is not None:
            self._group.close()  # its device workspace, now: not whenever the object is collected
            self._group = None

    def close(self) -> None:
        """Releases the group's device workspace and every tenant's engine."""
        self._drop_group()
        for s in self.tenants.values():
            if getattr(s, "engine", None) is not None:
                s.engine.close()
        self.tenants = {}

    def _tenant(self, name) -> CorpusServer:
        if name not in self.tenants:
            raise ValueError(f"unknown tenant {name!r}")
        return self.tenants[name]

    def load(self, name, bodies, ids) -> int:
        return self._tenant(name).load(bodies, ids)

    def append(self, name, bodies, ids) -> int:
        return self._tenant(name).append(bodies, ids)

    def rekey(self, name, eval_keys: dict) -> None:
        """CorpusServer.rekey of the tenant (its one-old-generation rules: a
        multi-bridge dict of §8.17 is refused, the group's bridge reads one
        key per tenant); the group re-reads the tenant's keys at the next call.
        With rotation_schedules any dict goes to the tenant's server, whose
        rules and messages apply with the tenant's name in front."""
        if self.rotation_schedules:
            server = self._tenant(name)
            try:
                return server.rekey(eval_keys)
            except ValueError as e:
                raise ValueError(f"tenant {name!r}: {e}") from e
        if "bridge_keys" in eval_keys or "bridge_key_bodies" in eval_keys:
            raise ValueError(f"tenant {name!r}: the hub keeps one old generation per tenant; a multi-bridge "
                             "dict needs a CorpusServer of its own")
        self._tenant(name).rekey(eval_keys)

    @staticmethod
    def gen_map(server) -> tuple:
        """(gen_ends, gen_slots) of a tenant's resident old generations: its
        several generations' ends and slots, else its one old generation in
        slot 0, else empty."""
        if getattr(server, "_old_gens", None):
            return [int(e) for _, e in server._old_gens], [int(s) for s in server._gen_slots]
        if int(getattr(server, "b_old", 0)):
            return [int(server.b_old)], [0]
        return [], []

    def group(self):
        if self._group is None:
            from .engine import EngineGroup
            self._group = EngineGroup([s.engine for s in self.tenants.values()])
        return self._group

    def rounds(self, requests: dict) -> list:
        """corpus_rounds of this hub's tenants (planning only)."""
        for name in requests:
            if self._tenant(name).body is None:
                raise ValueError(f"tenant {name!r} has no documents loaded")
        return corpus_rounds(requests, {n: self.tenants[n]._plan for n in requests},
                             {n: int(self.tenants[n].body.shape[0]) for n in requests})

    def search_many(self, requests: dict) -> dict:
        """requests: {name: (queries, min_similarity)} -> {name: [replies]},
        version-2 replies for the tenant's CorpusClient.decrypt_replies, its
        queries in order. A round's replies carry the round's width P. A
        group round sets EVERY tenant's engine to P, those that sit out too
        (a group needs one msg_bits); after a call that ran one, all engines
        are set back to P0. A tenant's own CorpusServer sets its width per
        chunk anyway, so results never depend on what a call left behind."""
        out = {name: [] for name in requests}
        names = list(self.tenants)
        grouped = False
        for rnd in self.rounds(requests):
            if rnd["mode"] == "own":
                for p in rnd["parts"]:
                    queries, min_similarity = requests[p["name"]]
                    q = np.atleast_2d(np.asarray(queries))
                    ts = thresholds_for(min_similarity, q.shape[0])
                    rng = p["queries"]
                    out[p["name"]] += self.tenants[p["name"]].search_many(q[rng.start:rng.stop], [ts[i] for i in rng])
                continue
            P = rnd["P"]
            grouped = True
            for s in self.tenants.values():  # a group needs one msg_bits on every context
                s.engine.set_msg_bits(P)
            items = [None] * len(names)
            for p in rnd["parts"]:
                s = self.tenants[p["name"]]
                last = self.gen_map(s) if self.rotation_schedules else (s.b_old,)
                items[names.index(p["name"])] = (s.body, s.ids, s.mask_key, s.engine.to_dev(p["W"]), p["cst"], p["Ts"],
                                                 s.bit_levels) + last
            if self.rotation_schedules:  # every tenant's old generations in one grouped bridge (§8.18)
                res = self.group().search_seeded_queries_gens(items)
            else:
                res = self.group().search_seeded_queries(items)
            for p in rnd["parts"]:
                ga, gb = res[names.index(p["name"])]
                B = int(self.tenants[p["name"]].body.shape[0])
                out[p["name"]].append(pack_replies(ga.cpu().numpy().view(np.uint64), gb.cpu().numpy().view(np.uint64),
                                                   B, P, p["Ts"]))
        if grouped:
            for s in self.tenants.values():
                s.engine.set_msg_bits(s.P0)
        return out
