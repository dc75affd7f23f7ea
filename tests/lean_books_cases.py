"""The shapes of tests/test_gpu_lean_books.py, in a module of their own so that tests/test_lean_books_args.py can hold them to what
they are for on the oracle alone, without a GPU.  No test lives here, and nothing here loads the library."""
NSF, RING34 = "nsfnet_chen_5-paths_6-modulations", "ring34_3-paths_6-modulations"
SEED = 31
B = 6                        # one full quad and one quad with two idle rows
EPISODE = 11                 # an episode ends every 10 steps: the reset counts the pending request as the next episode's first
LAUNCHES = (16, 40, 300)
CHUNKS = 7                   # ORLG_GROUP_CHUNKS of the cases that force chunks
# 140 steps in 7 chunks are chunks of 20 steps: every second episode ends on a chunk's last step
BOUNDARY_LAUNCHES = (140, 16)
CHUNK_STEPS = 20
# bit-rate tables of 16, 17, 32 and 33 entries: the lean body keeps two bit rates on each of a row's sixteen lanes (the second from
# index 16 on), and a handle of more than 32 takes the full body
RATE_COUNTS = (16, 17, 32, 33)
LEAN_MAX_RATES = 32


def rates(n):
    return tuple(25 * k for k in range(1, n + 1))


def kwargs(S=320, load=300, seed=SEED, **more):
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=EPISODE, seed=seed, **more)
