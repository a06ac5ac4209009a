"""tests/test_gpu_chain_classes.py on the emulated workgroup: the whole set - all seven classes on both paths - in one batch, and the query read alone and at the
end of a batch of two (half a minute each).  The default run leaves out the four reruns under the debug switches that force the chain stage's fallbacks
(seq_chain, dp_nospec, dp_seqtail, dp_serial: another half minute each); HAO_SIMT_FULL=1 runs them."""
from simt_suite import reexport, FULL

reexport(globals(), "test_gpu_chain_classes", skip=() if FULL else ("test_fallbacks_at_the_edges",))
