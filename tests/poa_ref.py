"""A plain partial-order alignment, written from the prose of include/cw_policy.h alone: global alignment with the three scores, the traceback preference,
the end cell, the incremental rank order and the column-majority consensus.  Dictionaries and lists for the graph, one int64 numpy row per node for the
DP (the horizontal move as a running maximum).  It shares no code with oracle/ or with the engine: tests/test_poa_ref_cpu.py holds it against the oracle,
tests/test_gpu_poa_routes.py holds the engine against it.  Besides the consensus it returns, after every member, what the probe catalogue
(tests/poa_probes.py) needs to prove which capacity or row kind a probe crosses.  Test infrastructure only."""
import collections

import numpy as np

MATCH, MISMATCH, GAP = 5, -4, -8  # cw_policy.h CW_POA_MATCH / CW_POA_MISMATCH / CW_POA_GAP (the default build)
CODES = "ACGT"

MemberStats = collections.namedtuple("MemberStats", "nodes edges max_indeg max_far new_nodes new_edges")
# nodes, edges: the graph after the member.  max_indeg: its largest in-degree.  max_far: the largest rank distance from a node to one of its predecessors.
# new_nodes, new_edges: what the member added (both 0: it walked an existing path).


class Graph:
    def __init__(self):
        self.base = []  # node -> its base
        self.inn = []  # node -> predecessors, in the order their edges were inserted
        self.out = []  # node -> successors
        self.col = []  # node -> its column (an id: the first node of the column)
        self.members = {}  # column -> its nodes, in rank order
        self.count = []  # node -> sequences through it
        self.order = []  # rank -> node
        self.edges = 0
        self.first = {}  # column -> the first sequence's node in it
        self.n_seq = 0

    def _node(self, base, col, at):
        v = len(self.base)
        self.base.append(base)
        self.inn.append([])
        self.out.append([])
        self.count.append(0)
        self.col.append(v if col is None else col)
        self.members.setdefault(self.col[v], [])
        self.order.insert(at, v)
        return v

    def ranks(self):
        return {v: r for r, v in enumerate(self.order)}

    def align(self, seq):
        """[(node or None, position in seq or None)] from the first cell to the end cell."""
        n, L = len(self.order), len(seq)
        rank = self.ranks()
        s = np.frombuffer(seq.encode(), np.uint8)
        score = {b: np.where(s == ord(b), MATCH, MISMATCH).astype(np.int64) for b in CODES}
        ramp = GAP * np.arange(L + 1, dtype=np.int64)
        H = np.empty((n + 1, L + 1), np.int64)  # row 0: before any node; row r + 1: the node of rank r
        H[0] = ramp
        rows = []
        for r, v in enumerate(self.order):
            pr = [rank[p] + 1 for p in self.inn[v]] or [0]
            rows.append(pr)
            if len(pr) == 1:
                up = H[pr[0]]
            else:
                up = H[pr].max(axis=0)
            V = up + GAP  # vertical: the node against a gap
            np.maximum(V[1:], up[:-1] + score[self.base[v]], out=V[1:])  # diagonal
            V -= ramp
            np.maximum.accumulate(V, out=V)  # horizontal: a base against a gap
            H[r + 1] = V + ramp
        # end cell: the sink of lowest rank among those with the best last-column score
        end, best = None, None
        for r, v in enumerate(self.order):
            if not self.out[v] and (best is None or H[r + 1, L] > best):
                end, best = r + 1, H[r + 1, L]
        path, i, j = [], end, L
        while i > 0 or j > 0:
            if i == 0:
                j -= 1
                path.append((None, j))
                continue
            v, h = self.order[i - 1], H[i, j]
            step = None
            if j > 0:
                sc = score[self.base[v]][j - 1]
                for p in rows[i - 1]:
                    if H[p, j - 1] + sc == h:
                        step = (p, j - 1, (v, j - 1))
                        break
            if step is None:
                for p in rows[i - 1]:
                    if H[p, j] + GAP == h:
                        step = (p, j, (v, None))
                        break
            if step is None:
                assert j > 0 and H[i, j - 1] + GAP == h
                step = (i, j - 1, (None, j - 1))
            i, j = step[0], step[1]
            path.append(step[2])
        path.reverse()
        return path

    def add(self, seq):
        n0, e0 = len(self.base), self.edges
        if not self.order:
            path = [(None, j) for j in range(len(seq))]
        else:
            path = self.align(seq)
        placed = [(v, j) for v, j in path if j is not None]  # one entry per base of seq, in order
        assert [j for _, j in placed] == list(range(len(seq)))
        nodes = [None] * len(seq)
        # matches and mismatches first: every base aligned to a node joins that node's column
        for v, j in placed:
            if v is None:
                continue
            c = self.col[v]
            same = [u for u in self.members[c] if self.base[u] == seq[j]]
            if same:
                nodes[j] = same[0]
            else:
                last = self.members[c][-1]
                u = self._node(seq[j], c, self.order.index(last) + 1)  # right after the last member of the column it joins
                self.members[c].append(u)
                nodes[j] = u
        # insertions: right before the first member of the column of the next path node that has a rank, at the very end if there is none
        for j in range(len(seq)):
            if nodes[j] is not None:
                continue
            nxt = next((nodes[k] for k in range(j + 1, len(seq)) if nodes[k] is not None), None)
            at = len(self.order) if nxt is None else self.order.index(self.members[self.col[nxt]][0])
            u = self._node(seq[j], None, at)
            self.members[u].append(u)
            nodes[j] = u
        for j, u in enumerate(nodes):
            self.count[u] += 1
            if self.n_seq == 0:
                self.first[self.col[u]] = u
            if j and nodes[j - 1] not in self.inn[u]:
                self.inn[u].append(nodes[j - 1])
                self.out[nodes[j - 1]].append(u)
                self.edges += 1
        self.n_seq += 1
        rank = self.ranks()
        far = max((rank[v] - rank[p] for v in range(len(self.base)) for p in self.inn[v]), default=0)
        assert all(rank[p] < rank[v] for v in range(len(self.base)) for p in self.inn[v]), "the rank order is not topological"
        return MemberStats(len(self.base), self.edges, max(len(x) for x in self.inn), far, len(self.base) - n0, self.edges - e0)

    def consensus(self):
        out, seen = [], set()
        for v in self.order:
            c = self.col[v]
            if c in seen:
                continue
            seen.add(c)
            counts = {}
            for u in self.members[c]:
                counts[self.base[u]] = counts.get(self.base[u], 0) + self.count[u]
            top = max(counts.values())
            if self.n_seq - sum(counts.values()) > top:  # gaps > every base count: the column is dropped
                continue
            tied = sorted((b for b in counts if counts[b] == top), key=CODES.index)
            tpl = self.base[self.first[c]] if c in self.first else None
            out.append(tpl if tpl in tied else tied[0])
        return "".join(out)


def poa(seqs):
    """(consensus, [MemberStats per member]) of the non-empty sequences `seqs`, the first being the template."""
    g = Graph()
    stats = [g.add(s) for s in seqs]
    return g.consensus(), stats


def consensus(seqs):
    seqs = [s for s in seqs if s]
    return "" if not seqs else seqs[0] if len(seqs) == 1 else poa(seqs)[0]
