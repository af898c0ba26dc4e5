"""Golden fixture for the soft (Polyak) target update, made by running the
reference's OWN DQNAgent.learn and DQNAgent.update_target_network_soft
(src/agents/dqn_agent.py:328-380, :389-399) under the torch-backed TensorFlow
shim (tests/golden/tf_shim.py), the recipe of make_learn_golden.py: the
reference file is imported only after its SHA-256 is checked, fp32, MSE.
TEST INFRASTRUCTURE ONLY: run by hand where the reference checkout is, never
under pytest; the tests read only the .npz it writes.

Like learn.npz this pins the reference's Python under the TF restatement, not
real TensorFlow: tf.function is a pass-through in the shim, and what the shim
lacks for update_target_network_soft -- Sequential.variables and arithmetic on
a Variable -- is added here, one float32 torch op per TF op:
    tau * v          -> float32(tau) * v            (one rounded f32 product)
    (1.0 - tau) * v  -> float32(1.0 - tau) * v      (Python subtracts in double,
                                                     TF converts the result once)
    a + b            -> one rounded f32 sum
which is the three-kernel sequence the device kernels restate (soft_el).

Run: one junction, nn_layers [128, 128], replay 300, epsilon 1 throughout,
200 loop steps = 73 learns; agent.tau = 0.01 and a target_update_frequency
larger than the run (no hard sync), so after every successful learn() the
reference's own update_target_network_soft() runs -- the call the reference
keeps commented out at :372-373.

Stored (soft_target.npz): the inputs (obs, rew, done), the actions, the losses,
the final online and target nets (Keras order), and -- on every STRIDE-th
parameter, to keep the file small -- the online net after learn 1 (w1) and the
target after the first soft update (t1); the initial weights are not stored:
dmdqn_amd.agent.keras_initial_weights(RandomState(init_seed), 128, 1) draws
the same values (asserted here).

Usage:  python tests/golden/make_soft_golden.py [--out tests/golden]
"""
import argparse
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_learn_golden as MG  # noqa: E402  (the SHA-checked import, initial weights, episode)
import tf_shim  # noqa: E402

TAU = 0.01
STEPS, BUF, TUF, SEED, INIT_SEED = 200, 300, 100000, 5, 9
STRIDE = 8


def extend_shim():
    """What update_target_network_soft needs beyond make_learn_golden's use of
    the shim (tf_shim.py itself is not edited)."""
    torch = tf_shim.torch
    f32 = torch.float32

    def scalar(x):
        return torch.tensor(float(x), dtype=f32)  # TF converts a Python float once

    def value(x):
        return x.t.detach() if isinstance(x, tf_shim.Variable) else x

    tf_shim.Sequential.variables = property(lambda self: self.trainable_variables)
    tf_shim.Variable.__rmul__ = lambda self, k: scalar(k) * self.t.detach()   # tf.multiply
    tf_shim.Variable.__mul__ = lambda self, k: self.t.detach() * scalar(k)
    tf_shim.Variable.__add__ = lambda self, o: self.t.detach() + value(o)     # tf.add
    tf_shim.Variable.__radd__ = lambda self, o: value(o) + self.t.detach()


def run(dq):
    tf_shim.SUMMARIES.clear()
    tfm = sys.modules["tensorflow"]
    tfm.keras.losses.MeanSquaredError = tf_shim.MeanSquaredError
    cfg = {"learning_rate": 0.001, "gamma": 0.99, "epsilon_start": 1.0, "epsilon_min": 0.01,
           "epsilon_decay_steps": 200000, "replay_buffer_size": BUF, "batch_size": 128,
           "target_update_frequency": TUF, "nn_layers": [128, 128]}
    agent = dq.DQNAgent(89, 4, "J_0_0", cfg)
    agent.tau = TAU  # the reference reads self.tau (:398) and never sets it
    rng = np.random.RandomState(INIT_SEED)
    w0 = MG.keras_init(rng)
    # (this tree goes last on sys.path: its src/ package must not shadow the
    # reference's, which _import_dqn has imported by now)
    sys.path.append(os.path.dirname(os.path.dirname(HERE)))
    from dmdqn_amd.agent import keras_initial_weights
    same = keras_initial_weights(np.random.RandomState(INIT_SEED), 128, 1)[0]
    assert np.array_equal(MG._flat(w0), same), "the tests rebuild w0 from INIT_SEED"
    agent.online_network.set_weights(w0)
    agent.target_network.set_weights(w0)
    obs, rew, done = MG.make_episode(rng, STEPS)
    random.seed(SEED)
    np.random.seed(SEED)
    actions = np.zeros(STEPS, np.int32)
    losses = np.full(STEPS, np.nan, np.float64)
    w1 = t1 = None
    for t in range(STEPS):
        s = obs[t][None]
        a = agent.select_action(tfm.convert_to_tensor(s, dtype=tfm.float32))
        actions[t] = int(a)
        agent.remember(s, int(a), float(rew[t]), obs[t + 1][None], bool(done[t]))
        loss = agent.learn()
        if loss is None:
            continue
        losses[t] = float(loss.detach().numpy())
        agent.update_target_network_soft()  # the reference's own method (:389-399)
        if agent.learn_step_counter == 1:
            w1 = MG._flat(agent.online_network.get_weights())
            t1 = MG._flat(agent.target_network.get_weights())
    assert agent.learn_step_counter < TUF  # no hard sync in the run
    return dict(obs=obs.astype(np.int8), rew=rew, done=done.astype(np.uint8), actions=actions,
                losses=losses, w1=w1[::STRIDE], t1=t1[::STRIDE],
                final_online=MG._flat(agent.online_network.get_weights()),
                final_target=MG._flat(agent.target_network.get_weights()),
                learn_steps=np.array([agent.learn_step_counter]),
                tau=np.array([TAU], np.float64),
                cfg=np.array([STEPS, BUF, TUF, SEED, INIT_SEED, STRIDE]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    out = os.path.abspath(args.out)
    import tempfile
    os.chdir(tempfile.mkdtemp(prefix="dmdqn_golden_"))  # log_config.py truncates ./replay_buffer.log
    sys.dont_write_bytecode = True
    import torch
    torch.set_num_threads(1)
    dq = MG._import_dqn()
    extend_shim()
    r = run(dq)
    print("learns", int(r["learn_steps"][0]), "last loss", r["losses"][-1])
    path = os.path.join(out, "soft_target.npz")
    np.savez_compressed(path, **r)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
