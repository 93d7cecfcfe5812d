"""Case builders and expected values for the tree verify step (omni_decode_attention_tree_kv4: 0 - 32 new tokens per sequence, each
seeing the past and its ancestors among the fresh keys; omni_kv4_prefill_write_at_pos: rotation at past + depth; omni_kv4_compact_rows):
numpy + oracle only, shared by the CPU and GPU tests.  Built on tests/paged_prefill_cases.py: the pools, block tables, fused rows
and the poisoning are its Case's; the rotation positions and the mask are the tree's."""
import numpy as np

from oracle import kv4
from tests import paged_prefill_cases as pc
from tests import verify_attn_cases as vc

D = pc.D
MAX_Q = 32


# ---- trees: parents[0] = -1, parents[i] < i -------------------------------------------------------------------------------------
def chain(n):
    return np.arange(-1, n - 1, dtype=np.int64)


def star(n):
    """every node a child of the root"""
    p = np.zeros(n, np.int64)
    p[0] = -1
    return p


def binary(n):
    return np.asarray([-1] + [(i - 1) // 2 for i in range(1, n)], np.int64)


def two_chains(n):
    """two chains off the root: the odd and the even nodes"""
    return np.asarray([-1] + [0 if i <= 2 else i - 2 for i in range(1, n)], np.int64)


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray([-1] + [int(rng.integers(0, i)) for i in range(1, n)], np.int64)


KINDS = ["chain", "star", "binary", "two_chains", "random"]


def tree(kind, n, seed=0):
    if n == 0:
        return np.zeros(0, np.int64)
    return {"chain": chain, "star": star, "binary": binary, "two_chains": two_chains,
            "random": lambda m: random_tree(m, seed)}[kind](n)


def masks_depths(parents):
    """(mask uint32 [n]: bit j = j is node i or one of its ancestors, depth int32 [n]), derived by walking up from every node."""
    n = len(parents)
    mask, depth = np.zeros(n, np.uint32), np.zeros(n, np.int32)
    for i in range(n):
        j, bits, d = i, 0, -1
        while j >= 0:
            bits |= 1 << j
            d += 1
            j = int(parents[j])
        mask[i], depth[i] = bits, d
    return mask, depth


# ---- a batch whose sequences carry a tree each -------------------------------------------------------------------------------------
class TreeCase(pc.Case):
    """pc.Case (pools, shuffled tables, fused rows) + one tree per sequence: qkv_rot is rotated at past + depth (v unchanged), mask
    holds the ancestor words in token order."""

    def __init__(self, triples, Hq, Hk, tpb, seed):
        """triples: (past, n, kind) per sequence"""
        super().__init__([(p, n) for p, n, _ in triples], Hq, Hk, tpb, seed)
        self.parents = [tree(kind, n, seed + 17 * b) for b, (_, n, kind) in enumerate(triples)]
        md = [masks_depths(p) for p in self.parents]
        self.mask = np.concatenate([m for m, _ in md] + [np.zeros(0, np.uint32)]).astype(np.uint32)
        self.depth = np.concatenate([d for _, d in md] + [np.zeros(0, np.int32)]).astype(np.int32)
        self.qkv_rot = rotate_at(self.qkv_raw, self.rope_positions(), Hq, Hk)

    def rope_positions(self):
        return np.repeat(self.pasts, self.lens).astype(np.int64) + self.depth


def rotate_at(qkv_raw, pos, Hq, Hk):
    """The fused rows with q and k rotated (neox) at the given position per token; v unchanged."""
    out = np.array(qkv_raw, np.float16, copy=True)
    T = out.shape[0]
    if T == 0:
        return out
    qk = out[:, : (Hq + Hk) * D].reshape(T, Hq + Hk, D)
    out[:, : (Hq + Hk) * D] = kv4.rope_neox(qk, np.broadcast_to(np.asarray(pos)[:, None], (T, Hq + Hk)), pc.ROPE_BASE).reshape(T, -1)
    return out


def write_at_pos(qkv_raw, lens, pasts, rope_pos, case):
    """Expected effect of omni_kv4_prefill_write_at_pos on the case's pools: rotation at rope_pos, slot past + i; -> rotated rows."""
    rot = rotate_at(qkv_raw, rope_pos, case.Hq, case.Hk)
    _, k, v = case.split(rot)
    slot_pos = pc.positions(lens, pasts)
    tok = 0
    for b, n in enumerate(lens):
        for _ in range(int(n)):
            p = int(slot_pos[tok])
            for h in range(case.Hk):
                case.kc.write_token(int(case.kidx[b][p // case.tpb]), p % case.tpb, h, k[tok, h])
                case.vc.write_token(int(case.vidx[b][p // case.tpb]), p % case.tpb, h, v[tok, h])
            tok += 1
    return rot


def expected_tree_attention(q, k_new, v_new, cu, pasts, mask, kc, vc_, kidx, vidx, with_mass=False):
    """f64 masked softmax per (sequence, token, head), as NeedleBatch.expected does: keys = dequantised past (exact fp16 values) +
    the fresh keys whose bit is set in the token's word (bits >= len_q ignored).  A row that sees nothing is zeros.
    -> fp16 [T, Hq, D] (and, with_mass, the probabilities of the fresh keys f64 [T, Hq, 32], 0 where not visible)."""
    T, Hq, _ = q.shape
    Hk = k_new.shape[1]
    G = Hq // Hk
    out = np.zeros((T, Hq, D), np.float64)
    mass = np.zeros((T, Hq, MAX_Q), np.float64)
    for b in range(len(pasts)):
        past, a, e = int(pasts[b]), int(cu[b]), int(cu[b + 1])
        n = e - a
        if n == 0:
            continue
        for hk in range(Hk):
            K = np.concatenate([kc.read_tokens(kidx[b], hk, past, fp16_math=True).astype(np.float64),
                                k_new[a:e, hk].astype(np.float64)])
            V = np.concatenate([vc_.read_tokens(vidx[b], hk, past, fp16_math=True).astype(np.float64),
                                v_new[a:e, hk].astype(np.float64)])
            for i in range(n):
                vis = np.concatenate([np.ones(past, bool), [(int(mask[a + i]) >> j) & 1 == 1 for j in range(n)]]).astype(bool)
                if not vis.any():
                    continue
                for h in range(hk * G, (hk + 1) * G):
                    s = K[vis] @ q[a + i, h].astype(np.float64) / np.sqrt(D)
                    p = np.exp(s - s.max())
                    p /= p.sum()
                    out[a + i, h] = p @ V[vis]
                    full = np.zeros(past + n)
                    full[vis] = p
                    mass[a + i, h, :n] = full[past:]
    out = out.astype(np.float16)
    return (out, mass) if with_mass else out


def case_expected(case):
    q, k, v = case.split(case.qkv_rot)
    return expected_tree_attention(q, k, v, case.cu, case.pasts, case.mask, case.kc, case.vc, case.kidx, case.vidx)


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
# Per GQA family (the four (Hq, Hk, tokens_per_block) of verify_attn_cases.FAMILIES): 12 sequences in ONE batch, pasts
# {0, 1, 63, 64, 65, 200} x 2 and n {1, 2, 8, 9, 17, 32} x 2, paired by a shift that differs per family so that the four families
# together meet every past with four different n; the tree kinds rotate along the batch (a different tree per sequence).  n = 32
# at ratios 8 and 7 = 256 and 224 rows: two row groups, the second ragged at 7; n = 9 at ratio 8 = 72 rows: a ragged last tile.
PASTS = [0, 1, 63, 64, 65, 200]
LENS = [1, 2, 8, 9, 17, 32]
SPLITS = [0, 1, 2, 3, 7]


def family_triples(shift):
    out = []
    for rep in range(2):
        for i, past in enumerate(PASTS):
            out.append((past, LENS[(i + shift + 3 * rep) % 6], KINDS[(i + 2 * rep + shift) % 5]))
    return out


FAMILIES = {name: (Hq, Hk, tpb, family_triples(s))
            for s, (name, (Hq, Hk, tpb, _)) in enumerate(sorted(vc.FAMILIES.items()))}
# len_q = 0 and past = 0 sequences among the others; (0, 1): a single node that sees only itself
MIXED_BATCH = [(0, 32, "binary"), (200, 0, "chain"), (65, 3, "star"), (0, 0, "chain"), (130, 1, "chain"), (17, 9, "random"),
               (0, 1, "chain")]


def family(name):
    Hq, Hk, tpb, triples = FAMILIES[name]
    return TreeCase(triples, Hq, Hk, tpb, seed=sum(map(ord, name)) + 2000)


def mixed():
    return TreeCase(MIXED_BATCH, 8, 2, 64, seed=231)


def chain_case():
    """chain trees with n <= 8: the inputs of the bit-identity check against omni_decode_attention_multi_kv4"""
    return TreeCase([(0, 8, "chain"), (200, 5, "chain"), (65, 3, "chain"), (0, 0, "chain"), (130, 1, "chain"), (17, 8, "chain"),
                     (64, 2, "chain")], 8, 2, 64, seed=233)


class SiblingNeedles:
    """NeedleBatch's construction (keys and values at 1.5 x the standard normal, all q rows of a sequence equal one key as the kernel
    sees it) with a STAR tree of n = 4 fresh nodes: node i sees fresh key 0 (the root) and itself, not its siblings.  Sequence b of
    the past + n sequences aims at key b: a page key for b < past, fresh key b - past behind it.  Rows of node i in sequence
    past + j with j != i, j >= 1, i >= 1 aim at a sibling they must NOT see (and so do the root's rows, i = 0, in every sequence
    past + j, j >= 1); the rows of sequence past + 0 aim at the root, which every node sees; node i's rows of sequence past + i aim
    at themselves."""

    def __init__(self, past=150, n=4, Hq=8, Hk=2, tpb=16, seed=77):
        nb = vc.NeedleBatch(past=past, n=n, Hq=Hq, Hk=Hk, tpb=tpb, seed=seed)
        self.__dict__.update(nb.__dict__)
        self.parents = star(n)
        m, d = masks_depths(self.parents)
        self.mask = np.tile(m, self.B).astype(np.uint32)
        self.depth = np.tile(d, self.B).astype(np.int32)

    def expected(self):
        """-> (fp16 [T, Hq, D], needle mass [B, n, Hq]: NaN where the row may not see its needle)"""
        want, fresh = expected_tree_attention(self.q, self.k_new, self.v_new, self.cu, self.pasts, self.mask, self.kc, self.vc,
                                              self.kidx, self.vidx, with_mass=True)
        B, n, Hq, past = self.B, self.n, self.Hq, self.past
        mass = np.full((B, n, Hq), np.nan)
        K = self.keys.astype(np.float64)
        q = self.q.astype(np.float64).reshape(B, n, Hq, D)
        G = Hq // self.Hk
        m, _ = masks_depths(self.parents)
        for b in range(B):
            for i in range(n):
                if b >= past:
                    if (int(m[i]) >> (b - past)) & 1:
                        mass[b, i] = fresh.reshape(B, n, Hq, MAX_Q)[b, i, :, b - past]
                    continue
                vis = np.concatenate([np.ones(past, bool), [(int(m[i]) >> j) & 1 == 1 for j in range(n)]])
                for h in range(Hq):
                    s = K[vis, h // G] @ q[b, i, h] / np.sqrt(D)
                    p = np.exp(s - s.max())
                    mass[b, i, h] = p[b] / p.sum()
        return want, mass


# ---- compaction ---------------------------------------------------------------------------------------------------------------------
def compact_expected(pool, idx, tpb, Hk, page_bytes, base, src, counts):
    """numpy move that snapshots first: for every sequence, head and j < counts[b] the row (64 code bytes, scale, zero) at position
    base[b] + src[b][j] -> base[b] + j.  pool uint8 [pages, page_bytes]; idx [B, pages] page indices.  -> new pool."""
    snap = pool.copy()
    out = pool.copy()
    data = Hk * tpb * (D // 2)

    def views(arr, page):
        return (arr[page, :data].reshape(Hk, tpb, D // 2), arr[page, data: data + Hk * tpb * 2].reshape(Hk, tpb, 2),
                arr[page, data + Hk * tpb * 2: data + Hk * tpb * 4].reshape(Hk, tpb, 2))
    for b in range(len(base)):
        for j in range(int(counts[b])):
            s, d = int(base[b]) + int(src[b][j]), int(base[b]) + j
            sv, dv = views(snap, int(idx[b][s // tpb])), views(out, int(idx[b][d // tpb]))
            for a, c in zip(sv, dv):
                c[:, d % tpb] = a[:, s % tpb]
    return out
