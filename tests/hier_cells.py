"""The cell list of a hierarchical net (yolo3_darknet53 with new_model / hierarchical / h_join_type='max'), built from the
single-frame graph of oracle/train_cells64.py: the same cells in the same order, each with its frame multiplier `fm`
(the cell runs on B * fm frames and its BatchNorm counts B * fm * H * W samples), and a pool node "hpool.i" in front of
each of the first n stride-2 convs, which then reads the pooled plane.

A pool node is dict(name, pool=True, src=[pre-pool producer], cin, cout, fm, skip=None): fm is the consumer's, a third of
its producer's.  With four pools "hpool.3" is route 0: stages.1.0 and the stride-8 head (yolo_blocks.2.body.0, behind the
upsampled transition) both read it."""
from oracle import train_cells64 as R

VALID = ([3, 1, 1, 1, 1], [3, 3, 1, 1, 1], [3, 3, 3, 1, 1], [3, 3, 3, 3, 1])
# the stride-2 convs a pool stands in front of: after features[0], [1:3], [3:6], [6:15] (h_darknet.py:103-188)
POOL_CONSUMERS = ("stages.0.1", "stages.0.3", "stages.0.6", "stages.1.0")


def n_pools(hierarchical):
    h = [int(v) for v in hierarchical]
    if h not in [list(v) for v in VALID]:
        raise ValueError("not a hierarchical list the reference can run: %r" % (hierarchical,))
    return h.index(1)


def hier_graph(num_class, hierarchical):
    n = n_pools(hierarchical)
    fm = 3 ** n
    out, renamed = [], {}
    for c in R.graph(num_class):
        c = dict(c)
        if c["name"] in POOL_CONSUMERS[:n]:
            i = POOL_CONSUMERS.index(c["name"])
            (src,) = c["src"]
            fm //= 3
            out.append(dict(name="hpool.%d" % i, pool=True, src=[src], cin=c["cin"], cout=c["cin"], fm=fm, skip=None))
            renamed[src] = "hpool.%d" % i
        # every later reader of a pooled producer reads the pooled plane (the pre-pool plane's only consumer is the pool)
        c["src"] = [renamed.get(p, p) for p in c["src"]]
        assert c["skip"] not in renamed, c["name"]
        c["fm"] = fm if c["name"].startswith("stages.") else 1
        out.append(c)
    assert fm == 1
    return out
