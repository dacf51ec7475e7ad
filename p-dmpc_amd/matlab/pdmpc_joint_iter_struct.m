function s = pdmpc_joint_iter_struct(iter)
    % PDMPC_JOINT_ITER_STRUCT  The IterationData of all iter.amount vehicles (IterationData.m:4-33) as the struct
    % pdmpc_mex('plan_joint', ...) reads: row v of every per-vehicle field is vehicle v; the obstacles are the scenario's,
    % shared by the vehicles.  Nothing is flattened here: include/pdmpc_matlab.h (pdmpc_ml_joint_iter) and
    % csrc/matlab_marshal.cpp do that.
    boundary = {};

    if ~isempty(iter.predicted_lanelet_boundary)
        boundary = iter.predicted_lanelet_boundary(:, 1:2); % N x 2 cell: left, right
    end

    s = struct( ...
        'x0', iter.x0, ... % N x 4
        'trim_indices', iter.trim_indices(:), ...
        'reference_trajectory_points', iter.reference_trajectory_points, ... % N x Hp x 2
        'v_ref', iter.v_ref, ... % N x Hp
        'predicted_lanelet_boundary', {boundary}, ...
        'obstacles', {iter.obstacles}, ...
        'dynamic_obstacle_area', {iter.dynamic_obstacle_area} ... % n_d x Hp cell
    );
end
