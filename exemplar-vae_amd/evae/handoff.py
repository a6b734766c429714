"""What the runner of one training step (evae/graph.py) tells the model (models/BaseModel.py) and the fused node (evae/fused_vae.py,
ops.prior_logp on the modular paths) about THIS step, and the one thing the node tells it back.  calculate_loss and
get_exemplar_set keep the reference's signatures, so none of it can be an argument: the runner installs ONE StepHandoff for the
length of the step, the others look at current().  The slot is a plain module global on purpose: autograd runs backward functions
on a thread of its own, and one that looks must see the step's object (a thread-local would show it None).  No torch at import."""
import contextlib

_current = None


class DropoutSource:
    """The dropout masks of ONE step of a runner: `seed_ctr`, the two device words [seed, step counter] of its control block, and
    the ordinal the next mask of the step takes (0, 1, 2, ... in the order the forward pass asks; a backward pass reuses the
    ordinal of its forward, evae/ops.py).  A replayed launch carries the pointer and its ordinal; the counter is the replay's."""
    __slots__ = ("seed_ctr", "ordinal")

    def __init__(self, seed_ctr):
        self.seed_ctr, self.ordinal = seed_ctr, 0

    def take(self):
        o, self.ordinal = self.ordinal, self.ordinal + 1
        return o


class StepHandoff:
    __slots__ = ("rows", "n_rows", "dedup", "eps", "batch_staged", "unit_upstream", "beta", "prep", "wt", "p6", "p6_images", "dropout")

    def __init__(self, rows=None, n_rows=0, dedup=None):
        self.rows, self.n_rows = rows, n_rows   # gather list [this rank's exemplar rows | staging rows of the batch], rows of its head
        self.dedup = dedup                      # (draws, inv, rep, mult) when `rows` holds the DISTINCT rows of the draw only
        self.eps = None                         # the noise the step's prologue launch drew
        self.batch_staged = False               # the batch already sits in the store's staging rows
        # the only backward is loss.backward(ones) on the batch mean, and this is its beta as a device scalar (ops.prior_logp)
        self.unit_upstream, self.beta = False, None
        # what the step's head launch has done already, each honoured once and only for the pointers it was done for (take_*):
        # (prepared buffer, w1h, w1g): layer 1's weights are split; ((wm, w2h, w2g), buffers): the backward's transposed weights are
        # written; (w2h, w2g): both images of layer 2's weights are built
        self.prep = self.wt = self.p6 = None
        # back-channel: (w2h, w2g, H, forward image, data-gradient image) the node's pre-split layer 2 used in this step
        self.p6_images = None
        # a DropoutSource: the step's dropout calls take their masks from the control block (the pixelcnn decoder); None: the
        # process counter of ops.dropout_rng()
        self.dropout = None

    def take_prep(self, prep, w1h, w1g):
        tok, self.prep = self.prep, None
        return tok == (prep, w1h, w1g)

    def take_wt(self, wm, w2h, w2g):
        tok, self.wt = self.wt, None
        return tok[1] if tok is not None and tok[0] == (wm, w2h, w2g) else None

    def take_p6(self, w2h, w2g):
        tok, self.p6 = self.p6, None
        return tok == (w2h, w2g)


def current():
    """the hand-off of the step that is running, or None"""
    return _current


@contextlib.contextmanager
def active(h):
    """`h` is current() inside the block; on the way out, exception or not, the one before it is again, and no token of `h` is left"""
    global _current
    prev, _current = _current, h
    try:
        yield h
    finally:
        _current = prev
        h.prep = h.wt = h.p6 = None
