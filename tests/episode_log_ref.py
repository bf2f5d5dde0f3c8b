"""The logging loops of the reference's five collect_experiences, restated in numpy over recorded [T, N] arrays: list
appends, float32 running sums, the `keep` rule and the state an algo object carries from call to call.

  base       main/src/torch_ac/algos/base.py:167-182, 233-247
  hier       zone-goals/src/torch_ac/algos/_hier_policy_opt.py:79-93, 182-193
  options    options/src/torch_ac/algos/_hier_policy_opt.py:79-93, 176-188
  skills     main/src/torch_ac/algos/_hier_policy_opt.py:105-128, 216-232
  xy         xy-goals/src/torch_ac/algos/_hier_policy_opt.py:76-94, 178-191
"""
import numpy as np

VARIANTS = ("base", "hier", "options", "skills", "xy")
WINDOWED = ("skills", "xy")
f32 = np.float32


class EpisodeLogRef:
    """One algo object's log state.  ``collect`` is one call of collect_experiences' logging."""

    def __init__(self, num_procs, variant, skill_len=None):
        assert variant in VARIANTS
        assert (skill_len is not None) == (variant in WINDOWED)
        self.N, self.variant, self.L = int(num_procs), variant, skill_len
        N = self.N
        self.episode_return = np.zeros(N, f32)
        self.episode_reshaped_return = np.zeros(N, f32)
        self.episode_num_frames = np.zeros(N, f32)
        self.episode_diversity = np.zeros(N, f32)
        self.episode_prediction = np.zeros(N, f32)
        self.log_return = [0] * N
        self.log_reshaped_return = [0] * N
        self.log_num_frames = [0] * N
        self.log_diversity = [0] * N
        self.log_prediction = [0] * N
        self.log_env = [-1] * N

    def collect(self, reward, reshaped, done, diversity=None):
        """reward, reshaped, diversity: float32 [T, N], the frame's env reward, self.rewards[i] and the unscaled
        diversity reward; done: [T, N], the env's done of the frame.  Returns the call's ``logs`` (lists, as the reference
        returns them) with ``env_per_episode`` and ``done`` (log_done_counter) beside."""
        reward, reshaped = np.asarray(reward, f32), np.asarray(reshaped, f32)
        done = np.asarray(done) != 0
        T, N = reward.shape
        assert N == self.N and reshaped.shape == done.shape == (T, N)
        windowed = self.variant in WINDOWED
        if diversity is None:
            diversity = np.zeros((T, N), f32)
        diversity = np.asarray(diversity, f32)
        proc_active = [True] * N
        frame_counter = 0
        done_counter = 0
        for i in range(T):
            if windowed and i % self.L == 0:
                proc_active = [True] * N
            mask = (1 - done[i].astype(f32)).astype(f32)
            self.episode_return = (self.episode_return + reward[i]).astype(f32)
            self.episode_reshaped_return = (self.episode_reshaped_return + reshaped[i]).astype(f32)
            if self.variant == "skills":
                self.episode_diversity = (self.episode_diversity + diversity[i]).astype(f32)
            self.episode_num_frames = (self.episode_num_frames + np.ones(N, f32)).astype(f32)
            frame_counter += sum(proc_active)
            for j, done_ in enumerate(done[i]):
                if done_ and (proc_active[j] or not windowed):
                    if windowed:
                        proc_active[j] = False
                    done_counter += 1
                    self.log_return.append(self.episode_return[j].item())
                    self.log_reshaped_return.append(self.episode_reshaped_return[j].item())
                    self.log_num_frames.append(self.episode_num_frames[j].item())
                    self.log_diversity.append(self.episode_diversity[j].item())
                    self.log_prediction.append(self.episode_prediction[j].item())
                    self.log_env.append(j)
            self.episode_return = (self.episode_return * mask).astype(f32)
            self.episode_reshaped_return = (self.episode_reshaped_return * mask).astype(f32)
            self.episode_num_frames = (self.episode_num_frames * mask).astype(f32)
            self.episode_diversity = (self.episode_diversity * mask).astype(f32)
            self.episode_prediction = (self.episode_prediction * mask).astype(f32)
        keep = max(done_counter, N)
        logs = {"return_per_episode": self.log_return[-keep:],
                "reshaped_return_per_episode": self.log_reshaped_return[-keep:],
                "num_frames_per_episode": self.log_num_frames[-keep:],
                "num_frames": frame_counter if windowed else T * N,
                "env_per_episode": self.log_env[-keep:],
                "done": done_counter}
        if self.variant == "skills":
            logs["diversity_per_episode"] = self.log_diversity[-keep:]
        if windowed:
            logs["prediction_per_episode"] = self.log_prediction[-keep:]
        for name in ("log_return", "log_reshaped_return", "log_num_frames", "log_diversity", "log_prediction", "log_env"):
            setattr(self, name, getattr(self, name)[-N:])
        return logs


def done_from_masks(mask, next_mask):
    """done [T, N] from the recorded masks [T, N] (mask[t] = 1 - done of frame t - 1) and the mask the collector
    carries into its next call [N]."""
    mask = np.asarray(mask, f32)
    return np.concatenate([1 - mask[1:], 1 - np.asarray(next_mask, f32)[None]], axis=0) != 0
