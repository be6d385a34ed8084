"""The prefix trie of a list of candidate answers, for answer-list decoding of the generator heads (csrc/answer_trie.hip;
Decoder.answer_path_async, T5.constrained_greedy_async).  numpy only; torch is imported by `to_device` alone.

Entry i of the list is label i.  The trie is stored as CSR arrays, all int32:
  child_off  [N + 1]  the children of node n are entries child_off[n] .. child_off[n + 1] - 1
  child_tok  [E]      the token of an entry, ascending within a node
  child_node [E]      the node behind it
  leaf_label [N]      the label at the node behind an end token, -1 elsewhere
Node 0 is the root; nodes are numbered in breadth-first order and children in ascending token order, so the arrays are a function of
the list alone.  Every sequence ends with an end token and holds none before, so a leaf has no child and every other node has one:
a row of the search cannot get stuck.  The device follows the table unchecked (as lora.LoraTable): `to_device` is the check."""
import numpy as np

SCORE_MAX_DEPTH = 32    # the longest answer exhaustive list scoring takes: the key count of one wave pass of m3ae_tree_attn

class AnswerTrie:
    def __init__(self, sequences, end_ids):
        end_ids = (int(end_ids),) if np.isscalar(end_ids) else tuple(int(e) for e in end_ids)
        seqs = [tuple(int(t) for t in s) for s in sequences]
        if not seqs:
            raise ValueError("AnswerTrie: the answer list is empty")
        seen = {}
        for i, s in enumerate(seqs):
            if any(t < 0 for t in s):
                raise ValueError(f"AnswerTrie: answer {i} holds a negative token id")
            if not s or s[-1] not in end_ids:
                raise ValueError(f"AnswerTrie: answer {i} does not end with an end token {end_ids}")
            if any(t in end_ids for t in s[:-1]):
                raise ValueError(f"AnswerTrie: answer {i} holds an end token before its last position")
            if s in seen:
                raise ValueError(f"AnswerTrie: answers {seen[s]} and {i} are the same token sequence")
            seen[s] = i
        self.end_ids, self.sequences = end_ids, seqs
        self.num_answers = len(seqs)
        self.depth = max(len(s) for s in seqs)
        # breadth-first: a node is the set of answers that share a prefix; its children split that set by the next token
        child_off, child_tok, child_node, leaf_label = [0], [], [], [-1]
        queue = [(list(range(len(seqs))), 0)]      # (answers through the node, its depth), in node order
        head = 0
        while head < len(queue):
            members, d = queue[head]
            head += 1
            groups = {}
            for i in members:
                if len(seqs[i]) > d:
                    groups.setdefault(seqs[i][d], []).append(i)
            for tok in sorted(groups):
                g = groups[tok]
                child_tok.append(tok)
                child_node.append(len(queue))
                # behind an end token stands exactly one answer (no end token inside, no duplicates)
                leaf_label.append(g[0] if tok in end_ids else -1)
                queue.append((g, d + 1))
            child_off.append(len(child_tok))
        self.child_off = np.asarray(child_off, dtype=np.int32)
        self.child_tok = np.asarray(child_tok, dtype=np.int32)
        self.child_node = np.asarray(child_node, dtype=np.int32)
        self.leaf_label = np.asarray(leaf_label, dtype=np.int32)
        self.num_nodes, self.num_edges = len(leaf_label), len(child_tok)
        self.max_token = int(self.child_tok.max())
        self._uploaded = {}             # device -> the int32 trie buffer
        self._uploaded_answers = {}     # (device, max_len, pad_id) -> the int64 answers table
        self._score_tables = None       # score_tables(), built on first use
        self._uploaded_score = {}       # device -> the int32 buffer of the score tables
        self._uploaded_pen = {}         # device -> {length_penalty: the double table of len ** length_penalty}

    @classmethod
    def from_answers(cls, id_lists, end_id):
        """The trie of answers given without their end token: `end_id` is appended to each."""
        return cls([list(s) + [int(end_id)] for s in id_lists], (int(end_id),))

    def children(self, node):
        """(tokens, nodes) of a node's children."""
        lo, hi = int(self.child_off[node]), int(self.child_off[node + 1])
        return self.child_tok[lo:hi], self.child_node[lo:hi]

    def walk(self, seq):
        """The node reached from the root along `seq`, or -1 when the trie has no such path."""
        n = 0
        for t in seq:
            toks, nodes = self.children(n)
            j = int(np.searchsorted(toks, t))
            if j >= len(toks) or toks[j] != t:
                return -1
            n = int(nodes[j])
        return n

    def answers_table(self, max_len, pad_id):
        """The answers as a pad-filled int64 [A, max_len] array, row i = label i with its end token."""
        tab = np.full((self.num_answers, max_len), int(pad_id), dtype=np.int64)
        for i, s in enumerate(self.sequences):
            tab[i, :len(s)] = s
        return tab

    def score_tables(self):
        """The tables of exhaustive list scoring (csrc/tree_attn.hip, csrc/list_score.hip), a function of the list alone; all int32:
          parent    [N]           the parent node, -1 at the root
          depth     [N]           the node's depth, 0 at the root
          in_tok    [N]           the token on the edge into the node (-1 at the root: the start id is filled in at upload)
          internal  [Ni]          the nodes that have children, ascending -- breadth-first numbering, so ascending in depth too
          row_of    [N]           the inverse of `internal`, -1 at leaves
          anc       [Ni, depth]   for internal row i the internal rows from the root (first) to itself (last), then -1
          level_off [depth + 2]   the nodes of depth d are level_off[d] .. level_off[d + 1] - 1
          leaf_node [A]           the leaf of each label
        The edge into node n is entry n - 1 of child_tok / child_node: every edge makes one node, in the order the edges are made.
        ValueError if the longest answer has more than SCORE_MAX_DEPTH tokens (the depth cap of m3ae_tree_attn)."""
        if self._score_tables is not None:
            return self._score_tables
        if self.depth > SCORE_MAX_DEPTH:
            raise ValueError(f"AnswerTrie: the longest answer has {self.depth} tokens, list scoring has room for {SCORE_MAX_DEPTH}")
        N, D = self.num_nodes, self.depth
        if not np.array_equal(self.child_node, np.arange(1, N, dtype=np.int32)):
            raise ValueError("AnswerTrie: the nodes are not numbered in the order of their edges")
        parent = np.full(N, -1, dtype=np.int32)
        depth = np.zeros(N, dtype=np.int32)
        in_tok = np.full(N, -1, dtype=np.int32)
        counts = np.diff(self.child_off)
        parent[1:] = np.repeat(np.arange(N, dtype=np.int32), counts)
        in_tok[1:] = self.child_tok
        for n in range(1, N):                   # a parent precedes its children
            depth[n] = depth[parent[n]] + 1
        internal = np.flatnonzero(counts > 0).astype(np.int32)
        row_of = np.full(N, -1, dtype=np.int32)
        row_of[internal] = np.arange(len(internal), dtype=np.int32)
        anc = np.full((len(internal), D), -1, dtype=np.int32)
        for i, n in enumerate(internal):
            d = int(depth[n])
            anc[i, d] = i
            if d:
                anc[i, :d] = anc[row_of[parent[n]], :d]
        level_off = np.searchsorted(depth, np.arange(D + 2)).astype(np.int32)      # depth is non-decreasing in node order
        leaf_node = np.zeros(self.num_answers, dtype=np.int32)
        leaves = np.flatnonzero(self.leaf_label >= 0)
        leaf_node[self.leaf_label[leaves]] = leaves
        self._score_tables = dict(parent=parent, depth=depth, in_tok=in_tok, internal=internal, row_of=row_of, anc=anc,
                                  level_off=level_off, leaf_node=leaf_node)
        return self._score_tables

    def score_to_device(self, device, V, max_len, pad_id=0):
        """to_device(device, V, max_len, pad_id) plus the upload of score_tables(), once per device: the namespace also holds parent,
        node_depth, in_tok, internal, anc ([Ni, Dmax], Dmax = depth), level_off, leaf_node and Ni.  This upload is the range check the
        list-score kernels rely on (they still turn no table value into an address unchecked)."""
        import torch
        t = self.score_tables()
        ns = self.to_device(device, V, max_len, pad_id)
        device = torch.device(device)
        buf = self._uploaded_score.get(device)
        names = ("parent", "depth", "in_tok", "internal", "anc", "level_off", "leaf_node")
        if buf is None:
            host = torch.from_numpy(np.concatenate([t[n].reshape(-1) for n in names]))
            buf = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host
            self._uploaded_score[device] = buf
        o = 0
        for n in names:
            view = buf[o:o + t[n].size].view(t[n].shape)
            setattr(ns, "node_depth" if n == "depth" else n, view)
            o += t[n].size
        ns.Ni, ns.score_buf = len(t["internal"]), buf
        ns.pen = self._uploaded_pen.setdefault(device, {})     # length_penalty -> the double table len ** length_penalty (ops.listscore_fold)
        return ns

    def to_device(self, device, V, max_len, pad_id=None):
        """Uploads the arrays as one int32 buffer and returns a namespace of views of it (child_off, child_tok, child_node,
        leaf_label, buf, N, E, A, depth).  ValueError if a token is >= V or the longest answer exceeds max_len: the kernels follow
        the table as it is.  With `pad_id` the namespace also holds `answers`, the upload of answers_table(max_len, pad_id) (the
        beam search reads the token row of its best label from it)."""
        import torch
        from types import SimpleNamespace as NS
        if self.max_token >= V:
            raise ValueError(f"AnswerTrie: token {self.max_token} is outside a vocabulary of {V}")
        if self.depth > max_len:
            raise ValueError(f"AnswerTrie: the longest answer has {self.depth} tokens, the search has room for {max_len}")
        N, E = self.num_nodes, self.num_edges
        device = torch.device(device)
        buf = self._uploaded.get(device)
        if buf is None:             # one upload per device; from pinned memory, so that the copy does not make the host wait
            host = torch.from_numpy(np.concatenate([self.child_off, self.child_tok, self.child_node, self.leaf_label]))
            buf = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host
            self._uploaded[device] = buf
        o1, o2, o3 = N + 1, N + 1 + E, N + 1 + 2 * E
        ns = NS(child_off=buf[:o1], child_tok=buf[o1:o2], child_node=buf[o2:o3], leaf_label=buf[o3:], buf=buf, N=N, E=E,
                A=self.num_answers, depth=self.depth)
        if pad_id is not None:
            key = (device, int(max_len), int(pad_id))
            tab = self._uploaded_answers.get(key)
            if tab is None:
                host = torch.from_numpy(self.answers_table(max_len, pad_id))
                tab = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host
                self._uploaded_answers[key] = tab
            ns.answers = tab
        return ns
