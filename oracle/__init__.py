"""CPU oracle for the GraspLDM grasp-generation hot path.

TEST INFRASTRUCTURE ONLY.  Nothing under ``graspldm_amd/`` may import this
package; only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline``
leg of ``bench.py`` do, and there only as the checker / reported baseline.

Contents
--------
point_ops.c / cpu_backend.py  scalar C restatement of the reference's nine
                              forward CUDA kernels behind the 12 ``_backend``
                              names, pinned to the reference's own kernels
                              (tests/test_ref_kernels_gpu.py and the recorded
                              tests/golden/ref_point_ops.npz)
ref_build.py, ref_shim/       compile the reference's six point-op .cu files,
                              unmodified, as HIP for gfx950 into the
                              git-ignored oracle/_ref/ (two libraries: default
                              contraction and -ffp-contract=off)
ref_backend.py, ref_cases.py  ctypes front end of those libraries on CUDA
                              tensors; the cases they are compared on
record_ref_point_ops.py       GPU-only: writes tests/golden/ref_point_ops.npz
schedulers.py                 DDIM / DDPM step restated from the public
                              algorithm (diffusers is absent here: PARITY
                              UNPINNED at that third-party boundary)
torch_ref.py                  functional fp32 torch-CPU restatement of the
                              encoder / denoiser / decoder / sampler graph,
                              pinned by tests/golden/*.npz captured from the
                              reference's own Python (oracle/make_golden.py)
ref_import.py, make_golden.py container-only: import /root/reference with
                              shims and write the golden fixtures
"""
