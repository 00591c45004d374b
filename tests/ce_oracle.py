"""CPU checker of the community-enhanced model -- TEST INFRASTRUCTURE ONLY.

The oracle environment and featuriser (``oracle.refenv``) with a forward that takes the
three-column node input of ``CEMultiDismantler/MultiDismantler_net_graphsage.py:255-285``: a live
node's row is ``[dn, dn, c]`` (dn = residual degree / the layer's residual maximum, c the static
community prior), the virtual node's ``[1, 1, 0]``.  Past the input the network is the
unit-cost one, so every op and operand order below is ``oracle/refmodel.py``'s.
``tests/test_ce_oracle.py`` pins it to the reference's own CE rollouts.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import refenv, refmodel
from oracle.refmodel import EMB, spmm

MASK = refenv.MASK


def forward(w, deg, n2n, aux, prior, max_bp_iter=3):
    """Q of the live nodes of one graph; prior [2][n]: c of each live node per layer."""
    n = len(deg[0])
    node_input = torch.zeros((2, n, 3), dtype=torch.float)
    for l in range(2):
        d = torch.as_tensor(np.asarray(deg[l], dtype=np.float32)).reshape(n, 1)
        dmax, _ = torch.max(d, dim=0)
        dn = d / dmax
        c = torch.as_tensor(np.asarray(prior[l], dtype=np.float32)).reshape(n, 1)
        node_input[l] = torch.cat((dn, dn, c), axis=1)
    y_input = torch.cat((torch.ones((2, 1, 2), dtype=torch.float), torch.zeros((2, 1, 1), dtype=torch.float)), dim=2)
    sub_row = torch.zeros(n, dtype=torch.long)
    sub_col = torch.arange(n, dtype=torch.long)
    ones_n = torch.ones(n)
    embeds = []
    for l in range(2):
        row = torch.as_tensor(n2n[l][0], dtype=torch.long)
        col = torch.as_tensor(n2n[l][1], dtype=torch.long)
        val = torch.ones(row.numel())
        h = F.normalize(torch.relu(torch.matmul(node_input[l], w.w_n2l)), p=2, dim=1)
        y = F.normalize(torch.relu(torch.matmul(y_input[l], w.w_n2l)), p=2, dim=1)
        for _ in range(max_bp_iter):
            pool = spmm(row, col, val, n, h)
            node_lin = torch.matmul(pool, w.p1)
            ypool = spmm(sub_row, sub_col, ones_n, 1, h)
            y_node_lin = torch.matmul(ypool, w.p1)
            cur_lin = torch.matmul(h, w.p2)
            h = F.normalize(torch.relu(torch.matmul(torch.concat([node_lin, cur_lin], 1), w.p3)), p=2, dim=1)
            y_cur_lin = torch.matmul(y, w.p2)
            y = F.normalize(torch.relu(torch.matmul(torch.concat([y_node_lin, y_cur_lin], 1), w.p3)), p=2, dim=1)
        embeds.append(torch.cat((h, y), axis=0))
    msg = torch.zeros(2, n + 1, EMB)
    for l in range(2):
        msg[l] = refmodel._attention(w, embeds, l)
    hs = F.normalize(msg[:, :n, :], p=2, dim=2)
    ys = F.normalize(msg[:, n:, :], p=2, dim=2)
    aux_t = torch.as_tensor(np.asarray(aux, dtype=np.float32)).reshape(1, 2, 4)
    rep_row = torch.arange(n, dtype=torch.long)
    rep_col = torch.zeros(n, dtype=torch.long)
    q_list, w_layer = [], []
    for l in range(2):
        rep_y = spmm(rep_row, rep_col, ones_n, n, ys[l])
        outer = torch.matmul(torch.unsqueeze(hs[l], dim=2), torch.unsqueeze(rep_y, dim=1))
        cp = torch.reshape(torch.tile(w.cross, [n, 1]), [n, EMB, 1])
        emb = torch.reshape(torch.matmul(outer, cp), (n, EMB))
        hidden = torch.relu(torch.matmul(emb, w.h1))
        rep_aux = spmm(rep_row, rep_col, ones_n, n, aux_t[:, l, :])
        q_list.append(torch.matmul(torch.concat([hidden, rep_aux], 1), w.last_w))
        w_layer.append(torch.relu(rep_y @ w.wl1) @ w.wl2)
    mix = F.softmax(torch.concat(w_layer, dim=1), dim=1)
    q = mix[:, 0].unsqueeze(1) * q_list[0] + mix[:, 1].unsqueeze(1) * q_list[1]
    return q[:, 0].detach().numpy().copy()


def predict(weights, graph, covered, removed, prior):
    """Masked float64 Q row over all node ids; prior [2][N] over all nodes."""
    ids, deg, coo, aux, _ = refenv.featurize(graph, covered, removed)
    row = np.full(graph.num_nodes, MASK, dtype=np.float64)
    if ids:
        pr = [np.asarray(prior[l], dtype=np.float32)[np.asarray(ids)] for l in range(2)]
        row[np.asarray(ids)] = forward(weights, deg, coo, aux, pr).astype(np.float64)
    for k in covered:
        row[k] = MASK
    return row


def rollout(weights, graph, prior, step=1, on_predict=None, forced=None):
    """GetSol with the prior.  forced: a removal sequence to follow instead of the arg-sort
    (teacher forcing; every prediction is still made and handed to on_predict).
    Returns (score, sequence, ranks, maxcc)."""
    env = refenv.RefEnv(graph, "unit")
    sol = []
    t = 0
    while not env.terminal():
        q = predict(weights, graph, env.covered, env.removed, prior)
        if on_predict is not None:
            on_predict(t, q, env)
        t += 1
        if forced is not None:
            picks = forced[len(sol):len(sol) + step]
            if len(picks) == 0:
                raise AssertionError("the forced sequence ends before the terminal state")
        else:
            picks = np.argsort(-q)[:step]
        for a in picks:
            if env.terminal():
                break
            env.step(int(a))
            sol.append(int(a))
    return env.score, sol, env.ranks, env.maxcc
